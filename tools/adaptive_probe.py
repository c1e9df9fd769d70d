"""What adaptive sampling costs and saves against the single launch.

On config C4 (scene 2, 2048 x 2048, 1024 spp, depth 20, chunk 32), first level 32 (levels
32, 64, ... 1024), it measures

* the single launch (zrt_ctx_render_tiles): zrt_stats.render_ms and the device time of the
  whole enqueue between two events on the launch stream;
* a plain accumulation run (zrt_ctx_accum_*) in passes of the level sizes (32, 32, 64, ...
  512): what the same launches cost without the adaptive machinery.  --baseline-lib names
  the library this (and the single launch) is also measured with: the parent commit's build;
* adaptive runs (zrt_ctx_adapt_*) for a sweep of tolerances, 0 first (nothing may stop:
  the frame must hash to the committed C4 hash): render_ms, the device time from the first
  level's enqueue to the last level's end (the host's per-level waits for the surviving
  count lie inside it), the samples rendered as a fraction of the full frame's, and RMSE
  and largest absolute difference of the frame against the full 1024-spp frame rendered in
  the same process (which must hash to the committed C4 hash).  --map-tol T writes the
  sample-count map of tolerance T into --out as a grey PNG (samples / cap) and as text, one
  digit per tile.

Every measurement is a process of its own under `timeout` (a step that fails ends the tool),
in interleaved rounds.  One JSON per step under --out, and summary.json.

usage: python tools/adaptive_probe.py --out DIR [--baseline-lib PATH] [--rounds 2] [--reps 3]
                                      [--tols 0,0.0078125,...] [--map-tol 0.03125]
       python tools/adaptive_probe.py --step single|passes|TOL      (one measurement, JSON on stdout)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

C4 = {"scene": 2, "width": 2048, "height": 2048, "spp": 1024, "max_depth": 20, "traversal": "fast",
      "sample_chunk": 32}
FIRST = 32
TOLS = "0,0.00390625,0.0078125,0.015625,0.03125,0.0625,0.125"


def c4_hash():
    with open(os.path.join(REPO, "profiles", "frame_hashes.json")) as f:
        for e in json.load(f)["entries"]:
            if e["config"] == C4:
                return e["frame_sha1"]
    raise SystemExit("no C4 entry in profiles/frame_hashes.json")


def level_sizes(levels):
    return [b - a for a, b in zip([0] + levels[:-1], levels)]


def step(what, reps, map_path):
    import torch

    import zraytrace_amd as z
    s = z.load_scene(C4["scene"])
    p = z.RenderParams(C4["width"], C4["height"], C4["spp"], C4["max_depth"], sample_chunk=C4["sample_chunk"])
    ctx = z.RenderContext(s, p)
    n_tiles = ctx.tile_count(p)
    tiles = torch.zeros(n_tiles * 64 * 3, dtype=torch.float32, device="cuda")
    frame = torch.zeros(p.height * p.width * 3, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {"step": what, "build_id": z.build_id(), "config": C4, "runs": []}
    # (an older library, --baseline-lib, has no zrt_debug_adapt_plan: the levels restated)
    levels = [FIRST << k for k in range(16) if FIRST << k < p.samples_per_pixel] + [p.samples_per_pixel]
    if hasattr(z.lib(), "zrt_debug_adapt_plan"):
        assert z.adapt_plan(p, 0.0, FIRST) == levels
    out["levels"] = levels

    def read_frame():
        ctx.assemble(p, tiles.data_ptr(), frame.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        return frame.cpu().numpy().reshape(p.height, p.width, 3).copy()

    full = None
    if what not in ("single", "passes"):  # the full frame the adaptive one is compared with
        ctx.render_tiles(s.camera, p, tiles.data_ptr(), stream.cuda_stream)
        full = read_frame()
        out["full_sha1"] = hashlib.sha1(full.tobytes()).hexdigest()
    for rep in range(reps + 1):  # (the first is a warm-up: buffers are allocated in it)
        infos = []
        with torch.cuda.stream(stream):
            if what == "single":
                e0.record()
                ctx.render_tiles(s.camera, p, tiles.data_ptr(), stream.cuda_stream)
            elif what == "passes":
                e0.record()
                ctx.accum_begin(s.camera, p)
                for n in level_sizes(levels):
                    ctx.accum_pass(n, tiles.data_ptr(), stream.cuda_stream)
            else:
                ctx.adapt_begin(s.camera, p, float(what), FIRST)
                e0.record()
                while True:
                    infos.append(ctx.adapt_level(tiles.data_ptr(), stream.cuda_stream))
                    if infos[-1]["tiles_active_after"] == 0:
                        break
            e1.record()
        stream.synchronize()
        st = ctx.stats()
        if rep:
            out["runs"].append({"render_ms": round(st["render_ms"], 3), "schedule_ms": round(st["schedule_ms"], 3),
                                "device_ms": round(e0.elapsed_time(e1), 3)})
    img = read_frame()
    out["frame_sha1"] = hashlib.sha1(img.tobytes()).hexdigest()
    out["rays_processed"] = st["rays_processed"]
    out["samples_processed"] = st["samples_processed"]
    if full is not None:
        out["tolerance"] = float(what)
        out["level_infos"] = infos
        out["samples_fraction"] = st["samples_processed"] / (p.height * p.height * p.samples_per_pixel)
        d = (img.astype(np.float64) - full.astype(np.float64))[:, :p.height]
        out["rmse"] = float(np.sqrt((d * d).mean()))
        out["max_abs_diff"] = float(np.abs(d).max())
        per_tile = ctx.adapt_samples()
        out["tiles_at_level"] = {str(L): int((per_tile == L).sum()) for L in levels}
        if map_path:
            tx = (p.height + 7) // 8
            grid = per_tile.reshape(tx, tx).astype(np.float32) / np.float32(p.samples_per_pixel)
            grey = np.repeat(np.repeat(grid, 8, axis=0), 8, axis=1)[:p.height, :p.height]
            z.write_png(map_path, np.repeat(grey[:, :, None], 3, axis=2))
            # the same map as text (the record kept in the tree; the PNG is a by-product)
            digit = {L: str(k) for k, L in enumerate(levels)}
            with open(os.path.splitext(map_path)[0] + ".txt", "w") as f:
                f.write(f"# sample map of the C4 run at tolerance {what}: {tx} x {tx} tiles, top row first; "
                        f"digit k = level {levels} [k] samples per pixel\n")
                for row in per_tile.reshape(tx, tx)[::-1]:
                    f.write("".join(digit[int(v)] for v in row) + "\n")
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tols", default=TOLS)
    ap.add_argument("--map-tol")
    ap.add_argument("--map-path")
    ap.add_argument("--step-timeout", type=int, default=150)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps, a.map_path)
    if not a.out:
        ap.error("--out DIR")
    os.makedirs(a.out, exist_ok=True)
    want = c4_hash()
    steps = []
    if a.baseline_lib:
        steps += [("single-baseline", "single", a.baseline_lib), ("passes-baseline", "passes", a.baseline_lib)]
    steps += [("single", "single", None), ("passes", "passes", None)]
    steps += [(f"adapt-{t}", t, None) for t in a.tols.split(",")]
    results = {}
    for rnd in range(1, a.rounds + 1):
        for name, what, lib in steps:
            env = dict(os.environ)
            env.pop("ZRT_LIB", None)
            if lib:
                env["ZRT_LIB"] = os.path.abspath(lib)
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
                   "--step", what, "--reps", str(a.reps)]
            if a.map_tol and what == a.map_tol and rnd == 1:
                cmd += ["--map-path", os.path.join(a.out, f"samples-{what}.png")]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU after a failed step
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {name} (round {rnd}) failed with status {r.returncode}")
            d = json.loads(r.stdout.strip().splitlines()[-1])
            with open(os.path.join(a.out, f"{name}.{rnd}.json"), "w") as f:
                json.dump(d, f, indent=1)
            if "full_sha1" in d:
                assert d["full_sha1"] == want, f"{name}: the full frame {d['full_sha1']} is not the committed C4 frame"
            if d.get("samples_fraction", 1.0) == 1.0:  # nothing stopped before the cap
                assert d["frame_sha1"] == want, f"{name}: frame {d['frame_sha1']} is not the committed C4 frame {want}"
            results.setdefault(name, []).append(d)
            print(name, rnd, d["build_id"], [x["render_ms"] for x in d["runs"]], [x["device_ms"] for x in d["runs"]],
                  d.get("samples_fraction"), d.get("rmse"), d.get("max_abs_diff"), flush=True)
    summary = {"config": C4, "first_level": FIRST, "frame_sha1": want, "rows": {}}
    for name, ds in results.items():
        runs = [x for d in ds for x in d["runs"]]
        rm, dm = sorted(x["render_ms"] for x in runs), sorted(x["device_ms"] for x in runs)
        row = {"build_id": ds[0]["build_id"], "render_ms_median": rm[len(rm) // 2], "render_ms_min": rm[0],
               "render_ms_max": rm[-1], "device_ms_median": dm[len(dm) // 2], "device_ms_min": dm[0],
               "device_ms_max": dm[-1], "n": len(runs), "frame_sha1": ds[0]["frame_sha1"]}
        for k in ("tolerance", "samples_fraction", "rmse", "max_abs_diff", "tiles_at_level"):
            if k in ds[0]:
                row[k] = ds[0][k]
        if "level_infos" in ds[0]:
            row["levels_run"] = len(ds[0]["level_infos"])
        summary["rows"][name] = row
    with open(os.path.join(a.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary["rows"], indent=1))


if __name__ == "__main__":
    main()

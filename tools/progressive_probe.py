"""What rendering a frame in passes costs against the single launch.

On config C4 (scene 2, 2048 x 2048, 1024 spp, depth 20, chunk 32) it measures

* the single launch (zrt_ctx_render_tiles): zrt_stats.render_ms, and the device time
  of the whole enqueue (render + finalize) between two events on the launch stream;
* an accumulation run (zrt_ctx_accum_*) in passes of 1, 2, 4, 8 and 32 chunks: the
  run's render_ms (summed over its passes), the device time of the whole run (every
  pass's render + accumulate kernels) and the bytes of chunk sums a pass parks.

Every measurement is a process of its own under `timeout` (a step that fails ends the
tool), in interleaved rounds; --baseline-lib names the library the single launch is
also measured with (the parent commit's build).  Each final frame must hash to the
committed C4 hash (profiles/frame_hashes.json).  One JSON per step under --out, and
summary.json.

usage: python tools/progressive_probe.py --out DIR [--baseline-lib PATH] [--rounds 2] [--reps 3]
       python tools/progressive_probe.py --step single|CHUNKS      (one measurement, JSON on stdout)
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

C4 = {"scene": 2, "width": 2048, "height": 2048, "spp": 1024, "max_depth": 20, "traversal": "fast",
      "sample_chunk": 32}
PASS_CHUNKS = (1, 2, 4, 8, 32)


def c4_hash():
    with open(os.path.join(REPO, "profiles", "frame_hashes.json")) as f:
        for e in json.load(f)["entries"]:
            if e["config"] == C4:
                return e["frame_sha1"]
    raise SystemExit("no C4 entry in profiles/frame_hashes.json")


def step(what, reps):
    import torch

    import zraytrace_amd as z
    s = z.load_scene(C4["scene"])
    p = z.RenderParams(C4["width"], C4["height"], C4["spp"], C4["max_depth"], sample_chunk=C4["sample_chunk"])
    ctx = z.RenderContext(s, p)
    tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
    frame = torch.zeros(p.height * p.width * 3, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    chunk = p.sample_chunk or 32
    out = {"step": what, "build_id": z.build_id(), "config": C4, "runs": []}
    if what != "single":
        n = int(what) * chunk
        out["pass_samples"] = n
        out["passes"] = -(-p.samples_per_pixel // n)
        out["partial_bytes"] = z.debug_pass_plan(p, 0, n)["partial_bytes"]
    else:
        out["partial_bytes"] = ctx.tile_count(p) * 64 * (-(-p.samples_per_pixel // chunk)) * 16
    for rep in range(reps + 1):  # (the first is a warm-up: buffers are allocated in it)
        with torch.cuda.stream(stream):
            e0.record()
            if what == "single":
                ctx.render_tiles(s.camera, p, tiles.data_ptr(), stream.cuda_stream)
            else:
                ctx.accum_begin(s.camera, p)
                for done in range(0, p.samples_per_pixel, n):
                    ctx.accum_pass(min(n, p.samples_per_pixel - done), tiles.data_ptr(), stream.cuda_stream)
            e1.record()
        stream.synchronize()
        st = ctx.stats()
        if rep:
            out["runs"].append({"render_ms": round(st["render_ms"], 3), "schedule_ms": round(st["schedule_ms"], 3),
                                "device_ms": round(e0.elapsed_time(e1), 3)})
    ctx.assemble(p, tiles.data_ptr(), frame.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    img = frame.cpu().numpy().reshape(p.height, p.width, 3)
    out["frame_sha1"] = hashlib.sha1(img.tobytes()).hexdigest()
    out["rays_processed"] = st["rays_processed"]
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=150)
    a = ap.parse_args()
    if a.step:
        return step(a.step, a.reps)
    if not a.out:
        ap.error("--out DIR")
    os.makedirs(a.out, exist_ok=True)
    want = c4_hash()
    steps = [("single-baseline", "single", a.baseline_lib)] if a.baseline_lib else []
    steps += [("single", "single", None)] + [(f"pass{k}", str(k), None) for k in PASS_CHUNKS]
    results = {}
    for rnd in range(1, a.rounds + 1):
        for name, what, lib in steps:
            env = dict(os.environ)
            env.pop("ZRT_LIB", None)
            if lib:
                env["ZRT_LIB"] = os.path.abspath(lib)
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__),
                   "--step", what, "--reps", str(a.reps)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:  # nothing more is started on the GPU after a failed step
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"step {name} (round {rnd}) failed with status {r.returncode}")
            d = json.loads(r.stdout.strip().splitlines()[-1])
            with open(os.path.join(a.out, f"{name}.{rnd}.json"), "w") as f:
                json.dump(d, f, indent=1)
            assert d["frame_sha1"] == want, f"{name}: frame {d['frame_sha1']} is not the committed C4 frame {want}"
            results.setdefault(name, []).append(d)
            print(name, rnd, d["build_id"], [x["render_ms"] for x in d["runs"]], [x["device_ms"] for x in d["runs"]],
                  flush=True)
    summary = {"config": C4, "frame_sha1": want, "rows": {}}
    for name, ds in results.items():
        runs = [x for d in ds for x in d["runs"]]
        rm, dm = sorted(x["render_ms"] for x in runs), sorted(x["device_ms"] for x in runs)
        summary["rows"][name] = {
            "build_id": ds[0]["build_id"], "passes": ds[0].get("passes", 1), "partial_bytes": ds[0]["partial_bytes"],
            "render_ms_median": rm[len(rm) // 2], "render_ms_min": rm[0], "render_ms_max": rm[-1],
            "device_ms_median": dm[len(dm) // 2], "device_ms_min": dm[0], "device_ms_max": dm[-1], "n": len(runs)}
    with open(os.path.join(a.out, "summary.json"), "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary["rows"], indent=1))


if __name__ == "__main__":
    main()

"""The variance-guided filter's defaults and what it costs; the sibling
of tools/denoise_probe.py.

(a) defaults: for loaded scenes 1 and 2 and the "glass-inside" and "bubbles" scenes of
    tests/shading_scenes.py at 64 x 64, a 32-spp frame in chunks of 4 rendered as an
    accumulation run (frame, variance plane: zrt_ctx_accum_variance), its feature buffer and
    a 4096-spp frame are made once; then every point of a grid of powers of two per sigma
    (sigma_albedo and sigma_color also 0 = off), without and with ZRT_DN_DEMODULATE, is
    scored by the mean over the scenes of the RMSE of the guided-filtered frame
    (zrt_ctx_denoise_guided, the default iterations) against the 4096-spp frame.  The winner
    is the lowest mean among the points that lower every scene's RMSE (the condition of
    tests/test_gpu_denoise_guided.py).  The plain default filter (zrt_denoise_defaults) is
    scored on the same frames.  defaults.json; zrt_denoise_guided_defaults returns the winner
    (post.cpp ZRT_DG_*).
(b) bunny: config C4's frame (scene 2, 2048 x 2048) at 8 spp in chunks of 4: the device time
    of the plain default filter and of the guided default filter (zrt_ctx_denoise_ms),
    interleaved, the median of --reps calls each, and of zrt_ctx_accum_variance +
    zrt_ctx_assemble_plane.  bunny_2048.json.

Each step is a process of its own under `timeout`; a step that fails ends the tool.

usage: python tools/denoise_guided_probe.py --out DIR [--reps 5] [--only defaults|bunny]
       python tools/denoise_guided_probe.py --step defaults|bunny     (one step, JSON on stdout)
"""
import argparse
import itertools
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from denoise_probe import SCENES, rmse, scene_of, write_json  # noqa: E402

SIZE, SPP, CHUNK, REF_SPP, DEPTH = 64, 32, 4, 4096, 20
GRID = {"sigma_color": [0.0] + [2.0 ** k for k in range(0, 6)],
        "sigma_normal": [2.0 ** k for k in range(-5, 1)],
        "sigma_albedo": [0.0] + [2.0 ** k for k in (-12, -6, 0)],
        "sigma_depth": [2.0 ** k for k in range(-7, 0)],
        "flags": [0, 1]}
KEYS = list(GRID)


class Frame:
    """A scene's noisy frame, variance plane and features on the device, and its reference."""

    def __init__(self, z, key, w, h, spp, chunk, ref_spp):
        import dataclasses

        import torch
        self.key = key
        self.keep, view, cam = scene_of(z, key)
        self.p = p = z.RenderParams(w, h, spp, DEPTH, sample_chunk=chunk)
        self.ctx = ctx = z.RenderContext(view, p)
        n = ctx.tile_count(p)
        tiles = torch.zeros(n * 64 * 3, dtype=torch.float32, device="cuda")
        var_tiles = torch.zeros(n * 64, dtype=torch.float32, device="cuda")
        self.frame = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
        self.var = torch.zeros(h * w, dtype=torch.float32, device="cuda")
        self.feat = torch.zeros(h * w * 8, dtype=torch.float32, device="cuda")
        ctx.accum_begin(cam, p)
        ctx.accum_pass(spp, tiles.data_ptr())
        ctx.assemble(p, tiles.data_ptr(), self.frame.data_ptr())
        ctx.accum_variance(var_tiles.data_ptr())
        ctx.assemble_plane(p, var_tiles.data_ptr(), self.var.data_ptr())
        ctx.features(cam, p, self.feat.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        self.tiles, self.var_tiles, self.cam = tiles, var_tiles, cam
        self.noisy = self.frame.cpu().numpy().reshape(h, w, 3)
        if ref_spp:
            self.ref, _ = z.render(view, cam, dataclasses.replace(p, samples_per_pixel=ref_spp, sample_chunk=0))
            self.e_noisy = rmse(self.noisy, self.ref, h)


def step_defaults():
    import torch

    import zraytrace_amd as z
    from zraytrace_amd import _ffi
    data = [Frame(z, key, SIZE, SIZE, SPP, CHUNK, REF_SPP) for key in SCENES]
    out_dev = torch.zeros(SIZE * SIZE * 3, dtype=torch.float32, device="cuda")

    def score(run):
        errs = []
        for d in data:
            run(d)
            d.ctx.denoise_ms()
            torch.cuda.synchronize()
            errs.append(rmse(out_dev.cpu().numpy().reshape(SIZE, SIZE, 3), d.ref, SIZE))
        return errs

    plain_dn = z.denoise_defaults()
    plain = score(lambda d: d.ctx.denoise(d.p, plain_dn, d.frame.data_ptr(), d.feat.data_ptr(), out_dev.data_ptr()))
    rows = []
    for point in itertools.product(*[GRID[k] for k in KEYS]):
        dn = _ffi.Denoise(iterations=0, **dict(zip(KEYS[:4], point[:4])))
        errs = score(lambda d: d.ctx.denoise_guided(d.p, dn, point[4], d.frame.data_ptr(), d.feat.data_ptr(),
                                                    d.var.data_ptr(), out_dev.data_ptr()))
        rows.append({"point": list(point), "rmse": [round(e, 6) for e in errs], "mean": round(float(np.mean(errs)), 6),
                     "improves_all": all(e < d.e_noisy for e, d in zip(errs, data))})
    ok = [r for r in rows if r["improves_all"]]
    marg = {}
    for i, k in enumerate(KEYS):
        marg[k] = []
        for v in GRID[k]:
            sel = [r["mean"] for r in ok if r["point"][i] == v]
            marg[k].append([v, min(sel) if sel else None, len(sel)])
    top = [r["point"] + r["rmse"] + [r["mean"]] for r in sorted(ok, key=lambda r: r["mean"])[:10]]
    out = {"step": "defaults", "build_id": z.build_id(), "size": SIZE, "spp": SPP, "sample_chunk": CHUNK,
           "reference_spp": REF_SPP, "max_depth": DEPTH, "iterations": 5, "scenes": [str(k) for k in SCENES],
           "grid": GRID, "rmse_unfiltered": [round(d.e_noisy, 6) for d in data], "points": len(rows),
           "points_improving_every_scene": len(ok), "best_mean_any_point": min(rows, key=lambda r: r["mean"]),
           "plain_default_filter": {"sigmas": plain_dn.as_dict(), "rmse": [round(e, 6) for e in plain],
                                    "ratio": [round(e / d.e_noisy, 4) for e, d in zip(plain, data)],
                                    "mean": round(float(np.mean(plain)), 6)},
           "marginal_columns": ["value", "lowest mean among improving points", "improving points"],
           "marginals": marg, "top_columns": KEYS + ["rmse " + str(k) for k in SCENES] + ["mean"], "top": top}
    if ok:
        win = min(ok, key=lambda r: r["mean"])
        out["winner"] = {**dict(zip(KEYS, win["point"])), "iterations": 5}
        out["winner_rmse"] = win["rmse"]
        out["winner_ratio"] = [round(e / d.e_noisy, 4) for e, d in zip(win["rmse"], data)]
        out["winner_mean"] = win["mean"]
    else:
        out["best_ratio_per_scene"] = [round(min(r["rmse"][i] for r in rows) / d.e_noisy, 4)
                                       for i, d in enumerate(data)]
    for d in data:
        d.ctx.close()
    print(json.dumps(out))


def step_bunny(reps):
    import torch

    import zraytrace_amd as z
    w = h = 2048
    d = Frame(z, 2, w, h, 8, 4, 0)
    out_dev = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    out_var = torch.zeros(h * w, dtype=torch.float32, device="cuda")
    plain_dn = z.denoise_defaults()
    dn, flags = z.denoise_guided_defaults()
    runs = {
        "plain": lambda: d.ctx.denoise(d.p, plain_dn, d.frame.data_ptr(), d.feat.data_ptr(), out_dev.data_ptr()),
        "guided": lambda: d.ctx.denoise_guided(d.p, dn, flags, d.frame.data_ptr(), d.feat.data_ptr(),
                                               d.var.data_ptr(), out_dev.data_ptr()),
        "guided_no_demodulation": lambda: d.ctx.denoise_guided(d.p, dn, 0, d.frame.data_ptr(), d.feat.data_ptr(),
                                                               d.var.data_ptr(), out_dev.data_ptr()),
        "guided_with_out_variance": lambda: d.ctx.denoise_guided(d.p, dn, flags, d.frame.data_ptr(),
                                                                 d.feat.data_ptr(), d.var.data_ptr(),
                                                                 out_dev.data_ptr(), out_var.data_ptr()),
    }
    ms = {k: [] for k in runs}
    for rep in range(reps + 1):  # (the first round is a warm-up)
        for k, run in runs.items():
            run()
            t = d.ctx.denoise_ms()
            if rep:
                ms[k].append(round(t, 4))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    var_ms = []
    for rep in range(reps + 1):
        e0.record()
        d.ctx.accum_variance(d.var_tiles.data_ptr())
        d.ctx.assemble_plane(d.p, d.var_tiles.data_ptr(), d.var.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if rep:
            var_ms.append(round(e0.elapsed_time(e1), 4))
    out = {"step": "bunny", "build_id": z.build_id(), "width": w, "height": h, "spp": 8, "sample_chunk": 4,
           "max_depth": DEPTH, "reps": reps, "plain_sigmas": plain_dn.as_dict(), "guided_sigmas": dn.as_dict(),
           "guided_flags": flags, "denoise_ms": ms,
           "denoise_ms_median": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
           "variance_plane_ms": var_ms, "variance_plane_ms_median": round(float(np.median(var_ms)), 4),
           "variance_plane_note": "zrt_ctx_accum_variance + zrt_ctx_assemble_plane between two events on the "
                                  "default stream (the host-side table upload included)"}
    d.ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--only")
    a = ap.parse_args()
    if a.step == "defaults":
        return step_defaults()
    if a.step == "bunny":
        return step_bunny(a.reps)
    if not a.out:
        ap.error("--out DIR")
    os.makedirs(a.out, exist_ok=True)
    for name, fname in (("defaults", "defaults.json"), ("bunny", "bunny_2048.json")):
        if a.only and a.only != name:
            continue
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # nothing more is started on the GPU after a failed step
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"step {name} failed with status {r.returncode}")
        d = json.loads(r.stdout.strip().splitlines()[-1])
        write_json(os.path.join(a.out, fname), d)
        print(name, {k: v for k, v in d.items() if k not in ("marginals", "top", "grid")}, flush=True)


if __name__ == "__main__":
    main()

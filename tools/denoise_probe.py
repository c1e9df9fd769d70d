"""The denoiser's default sigmas and what the filter costs.

(a) defaults: for loaded scenes 1 and 2 and the "glass-inside" and "bubbles" scenes of
    tests/shading_scenes.py at 64 x 64, an 8-spp frame, its feature buffer
    (zrt_ctx_features) and a 4096-spp frame (z.render) are rendered once; then every point
    of a grid of powers of two per sigma is scored by the mean over the scenes of the RMSE
    of the filtered 8-spp frame (zrt_ctx_denoise, the default iterations) against the
    4096-spp frame.  The winner is the lowest mean among the points that lower every
    scene's RMSE (the quality condition of tests/test_gpu_denoise.py); the grid, the
    winner, its per-scene ratios, each sigma value's best score and the ten best points
    go to defaults.json.  zrt_denoise_defaults returns
    the winner (post.cpp ZRT_DN_SIGMA_*).
(b) bunny: config C4's frame (scene 2, 2048 x 2048) at 8 spp: the device time of
    zrt_ctx_features, of the render, and of zrt_ctx_denoise with the default sigmas for
    1 .. 8 iterations (zrt_ctx_denoise_ms, the median of --reps calls); iteration k's
    time is the difference of the totals of k + 1 and k iterations (the first total also
    holds the packing pass).  bunny_2048.json.

Each step is a process of its own under `timeout`; a step that fails ends the tool.

usage: python tools/denoise_probe.py --out DIR [--reps 5] [--only defaults|bunny]
       python tools/denoise_probe.py --step defaults|bunny     (one step, JSON on stdout)
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

SCENES = [1, 2, "glass-inside", "bubbles"]
SIZE, SPP, REF_SPP, DEPTH = 64, 8, 4096, 20
GRID = {"sigma_color": [2.0 ** k for k in range(-3, 3)],
        "sigma_normal": [2.0 ** k for k in range(-5, 1)],
        "sigma_albedo": [2.0 ** k for k in range(-12, 1)],
        "sigma_depth": [2.0 ** k for k in range(-7, 0)]}
KEYS = list(GRID)


def scene_of(z, key):
    if isinstance(key, int):
        s = z.load_scene(key)
        return s, s.view, s.camera
    import shading_scenes as S
    s, view, cam = S.get(key)
    return s, view, cam


def rmse(a, b, n):
    d = (a.astype(np.float64) - b.astype(np.float64))[:, :n]
    return float(np.sqrt((d * d).mean()))


def step_defaults():
    import dataclasses

    import torch

    import zraytrace_amd as z
    from zraytrace_amd import _ffi
    p = z.RenderParams(SIZE, SIZE, SPP, DEPTH)
    data = []
    for key in SCENES:
        keep, view, cam = scene_of(z, key)
        noisy, _ = z.render(view, cam, p)
        ref, _ = z.render(view, cam, dataclasses.replace(p, samples_per_pixel=REF_SPP))
        ctx = z.RenderContext(view, p)
        feat = torch.zeros(SIZE * SIZE * 8, dtype=torch.float32, device="cuda")
        ctx.features(cam, p, feat.data_ptr())
        ctx.sync()
        data.append({"key": key, "keep": keep, "ctx": ctx, "feat": feat, "ref": ref,
                     "noisy": torch.from_numpy(noisy).cuda(), "e_noisy": rmse(noisy, ref, SIZE)})
    out_dev = torch.zeros(SIZE * SIZE * 3, dtype=torch.float32, device="cuda")
    rows = []
    for point in itertools.product(*[GRID[k] for k in KEYS]):
        dn = _ffi.Denoise(iterations=0, **dict(zip(KEYS, point)))
        errs = []
        for d in data:
            d["ctx"].denoise(p, dn, d["noisy"].data_ptr(), d["feat"].data_ptr(), out_dev.data_ptr())
            d["ctx"].denoise_ms()
            torch.cuda.synchronize()
            errs.append(rmse(out_dev.cpu().numpy().reshape(SIZE, SIZE, 3), d["ref"], SIZE))
        rows.append({"point": list(point), "rmse": [round(e, 6) for e in errs], "mean": round(float(np.mean(errs)), 6),
                     "improves_all": all(e < d["e_noisy"] for e, d in zip(errs, data))})
    ok = [r for r in rows if r["improves_all"]]
    best_any = min(rows, key=lambda r: r["mean"])
    out_rows = summarise(rows)
    out = {"step": "defaults", "build_id": z.build_id(), "size": SIZE, "spp": SPP, "reference_spp": REF_SPP,
           "max_depth": DEPTH, "iterations": 5, "scenes": [str(k) for k in SCENES], "grid": GRID,
           "rmse_unfiltered": [round(d["e_noisy"], 6) for d in data], "points": len(rows),
           "points_improving_every_scene": len(ok), "best_mean_any_point": best_any,
           **out_rows}
    if ok:
        win = min(ok, key=lambda r: r["mean"])
        out["winner"] = dict(zip(KEYS, win["point"]))
        out["winner_rmse"] = win["rmse"]
        out["winner_ratio"] = [round(e / d["e_noisy"], 4) for e, d in zip(win["rmse"], data)]
    else:  # per scene: the best any point does, to decide which scene the condition cannot hold on
        out["best_ratio_per_scene"] = [round(min(r["rmse"][i] for r in rows) / d["e_noisy"], 4)
                                       for i, d in enumerate(data)]
    for d in data:
        d["ctx"].close()
    print(json.dumps(out))


def step_bunny(reps):
    import torch

    import zraytrace_amd as z
    s = z.load_scene(2)
    w = h = 2048
    p = z.RenderParams(w, h, SPP, DEPTH)
    ctx = z.RenderContext(s, p)
    n_tiles = ctx.tile_count(p)
    tiles = torch.zeros(n_tiles * 64 * 3, dtype=torch.float32, device="cuda")
    frame = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    out_dev = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
    feat = torch.zeros(h * w * 8, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    render_ms, feat_ms = [], []
    for rep in range(reps + 1):  # (the first is a warm-up: buffers are allocated in it)
        ctx.render_tiles(s.camera, p, tiles.data_ptr(), stream.cuda_stream)
        ctx.assemble(p, tiles.data_ptr(), frame.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        r = ctx.stats()["render_ms"]
        with torch.cuda.stream(stream):
            e0.record()
            ctx.features(s.camera, p, feat.data_ptr(), stream.cuda_stream)
            e1.record()
        stream.synchronize()
        ctx.sync()
        if rep:
            render_ms.append(round(r, 4))
            feat_ms.append(round(e0.elapsed_time(e1), 4))
    dn = z.denoise_defaults()
    totals = []
    for k in range(1, 9):
        dn.iterations = k
        ms = []
        for rep in range(reps + 1):
            ctx.denoise(p, dn, frame.data_ptr(), feat.data_ptr(), out_dev.data_ptr(), stream.cuda_stream)
            t = ctx.denoise_ms()
            if rep:
                ms.append(t)
        totals.append(round(float(np.median(ms)), 4))
    per_iter = [totals[0]] + [round(b - a, 4) for a, b in zip(totals[:-1], totals[1:])]
    px = w * h
    out = {"step": "bunny", "build_id": z.build_id(), "width": w, "height": h, "spp": SPP, "max_depth": DEPTH,
           "reps": reps, "render_ms": render_ms, "features_ms": feat_ms, "denoise_sigmas": dn.as_dict(),
           "denoise_total_ms_by_iterations": totals, "iteration_ms": per_iter,
           "iteration_ms_note": "entry 0 = packing pass + iteration 0 (step 1); entry k = total(k + 1) - total(k)",
           # what one iteration must move at least (each pixel's colour and features read once, its colour
           # written once) and what its 25 taps ask of the caches (3 x 16 B each)
           "bytes_min_per_iteration": px * (16 + 32 + 16), "bytes_tapped_per_iteration": px * 25 * 48}
    ctx.close()
    print(json.dumps(out))


def summarise(rows):
    """What is kept of the grid's scores (one row per point would be thousands of lines):
    per sigma and value, the lowest mean among the points with that value that lower every
    scene's RMSE and how many such points there are; and the ten best such points."""
    ok = [r for r in rows if r["improves_all"]]
    marg = {}
    for i, k in enumerate(KEYS):
        marg[k] = []
        for v in GRID[k]:
            sel = [r["mean"] for r in ok if r["point"][i] == v]
            marg[k].append([v, min(sel) if sel else None, len(sel)])
    top = [r["point"] + r["rmse"] + [r["mean"]] for r in sorted(ok, key=lambda r: r["mean"])[:10]]
    return {"marginal_columns": ["value", "lowest mean among improving points", "improving points"],
            "marginals": marg, "top_columns": KEYS + ["rmse " + str(k) for k in SCENES] + ["mean"], "top": top}


def write_json(path, d):
    """indent 1, with every list of scalars on one line."""
    import re
    text = json.dumps(d, indent=1)
    text = re.sub(r"\[[^\[\]{}]*\]", lambda m: re.sub(r"\s+", " ", m.group(0)).replace("[ ", "[").replace(" ]", "]"), text)
    with open(path, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=240)
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

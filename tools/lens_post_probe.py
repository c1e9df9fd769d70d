"""What the post chain of lens frames costs and what it gains (DESIGN.md section 5 "Denoising
lens frames"; zrt.h "denoising lens frames").  GPU box.

(a) timing: scene 2 (the bunny) at --size x --size through its camera's pose, FAST traversal:
    kernel ms (zrt_ctx_query_ms / zrt_ctx_camera_info / zrt_ctx_denoise_ms; min, median, max
    over --reps calls after a warm-up) of zrt_ctx_camera_features per lens model, of
    zrt_ctx_camera_moments against zrt_ctx_camera at 32 spp in chunks of 4 (interleaved), of
    zrt_ctx_camera_variance (events around the call) and of zrt_ctx_denoise_rect over the
    whole frame, plain and guided, beside zrt_ctx_denoise / zrt_ctx_denoise_guided on the
    same buffers (interleaved).  timing.json.
(b) quality: loaded scenes 1 and 2 and the "glass-inside" and "bubbles" scenes of
    tests/shading_scenes.py (tools/denoise_guided_probe.py's four) at 64 x 64 through a thin
    lens (aperture 0.1, focused at the camera's distance from the world origin) and a 120
    degree fisheye at the scene camera's pose: the RMSE against a 4096-spp lens frame of the
    noisy 32-spp frame (chunks of 4) and of its plain- and guided-filtered frames, both filters
    at their defaults, over the whole frame.  quality.json.

usage: python tools/lens_post_probe.py --out DIR [--size 2048] [--reps 5] [--only timing|quality]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from denoise_probe import SCENES, rmse, scene_of, write_json  # noqa: E402

SPP, CHUNK, REF_SPP, DEPTH, QSIZE = 32, 4, 4096, 20, 64
KINDS = ("pinhole", "thin", "ortho", "equirect", "fisheye")


def spread(ms):
    return {"min": min(ms), "median": float(np.median(ms)), "max": max(ms), "n": len(ms)}


def timing(size, reps):
    import torch

    import zraytrace_amd as z
    scene = z.load_scene(2)
    cam = scene.camera
    p = z.RenderParams(size, size, SPP, DEPTH, sample_chunk=CHUNK)
    ctx = z.RenderContext(scene, p)
    n = size * size
    sums, rgb, feat, var, out, out_var = (torch.zeros(n * k, dtype=torch.float32, device="cuda") for k in (4, 3, 8, 1, 3, 1))
    whole = z.rect(0, 0, size, size)
    q = z.camera_query(0, 0, size, size, SPP)
    rec = {"scene": 2, "size": size, "samples": SPP, "sample_chunk": CHUNK, "max_depth": DEPTH, "repeats": reps}
    focus = math.sqrt(cam.origin.x ** 2 + cam.origin.y ** 2 + cam.origin.z ** 2)
    lenses = {k: z.lens_from_camera(i, cam, aperture=0.02 if k == "thin" else 0.0, focus_dist=focus if k == "thin" else 0.0,
                                    fisheye_fov=120.0) for i, k in enumerate(KINDS)}

    def timed(launches):
        """{name: spread} of the launches, interleaved, after one warm-up round."""
        ms = {k: [] for k in launches}
        for i in range(reps + 1):
            for k, (launch, read) in launches.items():
                launch()
                ctx.sync()
                if i:
                    ms[k].append(read())
        return {k: spread(v) for k, v in ms.items()}

    rec["camera_features_ms"] = timed({k: ((lambda l=l: ctx.camera_features(p, l, whole, feat.data_ptr())), ctx.query_ms)
                                       for k, l in lenses.items()})
    pin = lenses["pinhole"]
    rec["camera_ms"] = timed({
        "zrt_ctx_camera": (lambda: ctx.camera(p, pin, q, sums.data_ptr(), rgb.data_ptr()), lambda: ctx.camera_info()["kernel_ms"]),
        "zrt_ctx_camera_moments": (lambda: ctx.camera_moments(p, pin, q, sums.data_ptr(), rgb.data_ptr()),
                                   lambda: ctx.camera_info()["kernel_ms"])})
    ctx.camera_features(p, pin, whole, feat.data_ptr())
    ctx.sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        ev[0].record()
        ctx.camera_variance(p, whole, SPP, sums.data_ptr(), var.data_ptr(), torch.cuda.current_stream().cuda_stream)
        ev[1].record()
        torch.cuda.synchronize()
        if i:
            ms.append(ev[0].elapsed_time(ev[1]))
    rec["camera_variance_ms"] = spread(ms)
    dn_p = z.denoise_defaults()
    dn_g, flags = z.denoise_guided_defaults()
    a = (rgb.data_ptr(), feat.data_ptr())
    rec["denoise_ms"] = timed({
        "zrt_ctx_denoise": (lambda: ctx.denoise(p, dn_p, *a, out.data_ptr()), ctx.denoise_ms),
        "zrt_ctx_denoise_rect, plain": (lambda: ctx.denoise_rect(p, dn_p, 0, whole, *a, 0, out.data_ptr()), ctx.denoise_ms),
        "zrt_ctx_denoise_guided": (lambda: ctx.denoise_guided(p, dn_g, flags, *a, var.data_ptr(), out.data_ptr(),
                                                              out_var.data_ptr()), ctx.denoise_ms),
        "zrt_ctx_denoise_rect, guided": (lambda: ctx.denoise_rect(p, dn_g, flags, whole, *a, var.data_ptr(), out.data_ptr(),
                                                                  out_var.data_ptr()), ctx.denoise_ms)})
    rec["denoise_iterations"], rec["guided_flags"] = dn_p.iterations, flags
    ctx.close()
    return rec


def quality():
    import dataclasses

    import zraytrace_amd as z
    rows = []
    for key in SCENES:
        keep, view, cam = scene_of(z, key)
        focus = math.sqrt(cam.origin.x ** 2 + cam.origin.y ** 2 + cam.origin.z ** 2)
        for model, lens in (("thin", z.lens_from_camera(z.ZRT_LENS_THIN, cam, aperture=0.1, focus_dist=focus)),
                            ("fisheye", z.lens_from_camera(z.ZRT_LENS_FISHEYE, cam, fisheye_fov=120.0))):
            p = z.RenderParams(QSIZE, QSIZE, SPP, DEPTH, sample_chunk=CHUNK)
            ref, _ = z.render_lens(view, dataclasses.replace(p, sample_chunk=0), lens, REF_SPP)
            guided, out = z.render_lens_denoised(view, p, lens, SPP)
            plain, _ = z.render_lens_denoised(view, p, lens, SPP, guided=False)
            row = {"scene": key, "lens": model, "rmse_noisy": rmse(out["noisy"], ref, QSIZE),
                   "rmse_plain": rmse(plain, ref, QSIZE), "rmse_guided": rmse(guided, ref, QSIZE)}
            row["plain_over_noisy"] = row["rmse_plain"] / row["rmse_noisy"]
            row["guided_over_noisy"] = row["rmse_guided"] / row["rmse_noisy"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    return {"size": QSIZE, "samples": SPP, "sample_chunk": CHUNK, "reference_samples": REF_SPP, "max_depth": DEPTH,
            "thin": {"aperture": 0.1, "focus_dist": "|camera origin|"}, "fisheye_fov": 120.0, "rows": rows,
            "mean": {k: float(np.mean([r[k] for r in rows])) for k in ("rmse_noisy", "rmse_plain", "rmse_guided")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["timing", "quality"])
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    import torch

    import zraytrace_amd as z
    stamp = {"build_id": z.build_id(), "device": torch.cuda.get_device_name(0)}
    if a.only != "quality":
        write_json(os.path.join(a.out, "timing.json"), {**timing(a.size, a.reps), **stamp})
    if a.only != "timing":
        write_json(os.path.join(a.out, "quality.json"), {**quality(), **stamp})


if __name__ == "__main__":
    main()

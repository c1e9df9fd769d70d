"""Measure the ray queries on a resident context (GPU box): any-hit against closest-hit
on ambient-occlusion rays, and a resident zrt_ctx_trace batch against one-shot zrt_trace.

Workload: origins at the first hits of a zrt_ctx_features buffer, directions
cosine-distributed about the normal, t_max = +inf and 0.25 x the scene's extent.
Kernel times are zrt_ctx_query_ms (HIP events around the query kernel), wall times
time.perf_counter around call + zrt_ctx_sync; every figure is min / median / max over
the repeats after warm-up launches.  Writes <out>/ao_scene<k>.json.

    python tools/query_probe.py [--scenes 2 6] [--traversals fast binary reference] [--size 1024] [--rays 1048576] [--out profiles/r15/queries]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch

import zraytrace_amd as z

F = np.float32
TRAVERSALS = (("fast", z.ZRT_TRAVERSAL_FAST), ("binary", z.ZRT_TRAVERSAL_BINARY), ("reference", z.ZRT_TRAVERSAL_REFERENCE))


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "n": len(xs)}


def ao_rays(ctx, scene, size, n_rays, seed=0):
    """(rays float32[n, 6], extent): n AO rays from the first hits of a size x size feature buffer."""
    p = z.RenderParams(size, size, 1, 1)
    feat = torch.zeros(size * size * 8, dtype=torch.float32, device="cuda")
    ctx.features(scene.camera, p, feat.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()
    f = feat.cpu().numpy().reshape(size, size, 8)
    cam = scene.camera
    v3 = lambda v: np.array([v.x, v.y, v.z], F)
    ys, xs = np.mgrid[0:size, 0:size]
    u = (xs.astype(F) / F(size))[..., None]
    v = (ys.astype(F) / F(size))[..., None]
    d = v3(cam.lower_left_corner) + v3(cam.horizontal) * u + v3(cam.vertical) * v - v3(cam.origin)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F)
    hit = f[..., 7].view(np.uint32) != 0
    pos = (v3(cam.origin) + d * f[..., 3:4]).astype(F)[hit]
    nrm = f[..., 0:3][hit]
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(pos), n_rays)
    w = rng.normal(size=(n_rays, 3))
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    dirs = (nrm[k] + F(0.999) * w).astype(F)  # cosine-distributed about the normal
    extent = float(np.linalg.norm(pos.max(0) - pos.min(0)))
    return np.ascontiguousarray(np.concatenate([pos[k], dirs], 1), F), extent


def time_kernels(ctx, p, rays_dev, n, t_max_dev, warm, reps):
    """(any-hit ms, closest-hit ms, occluded bool[n]) - zrt_ctx_query_ms of each kernel."""
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    t = torch.zeros(n, dtype=torch.float32, device="cuda")
    prim = torch.zeros(n, dtype=torch.int32, device="cuda")
    any_ms, hit_ms = [], []
    for i in range(warm + reps):
        ctx.occluded(p, rays_dev.data_ptr(), t_max_dev.data_ptr() if t_max_dev is not None else 0, n, out.data_ptr())
        ctx.sync()
        a = ctx.query_ms()
        ctx.trace(p, rays_dev.data_ptr(), n, t.data_ptr(), prim.data_ptr())
        ctx.sync()
        b = ctx.query_ms()
        if i >= warm:
            any_ms.append(a)
            hit_ms.append(b)
    return spread(any_ms), spread(hit_ms), out.cpu().numpy() != 0


def probe_scene(index, size, n_rays, warm, reps, traversals):
    scene = z.load_scene(index)
    p0 = z.RenderParams(1, 1, 1, 1)
    t0 = time.perf_counter()
    ctx = z.RenderContext(scene, p0)
    create_s = time.perf_counter() - t0
    rays, extent = ao_rays(ctx, scene, size, n_rays)
    n = len(rays)
    rays_dev = torch.from_numpy(rays).cuda()
    rec = {"scene": index, "n_prims": scene.n_prims, "rays": n, "feature_size": size, "scene_extent": extent,
           "context_create_s": create_s, "warmup": warm, "repeats": reps, "kernels": [], "resident_vs_one_shot": []}
    for label, t_max in (("inf", None), ("0.25 extent", 0.25 * extent)):
        tm = None if t_max is None else torch.full((n,), t_max, dtype=torch.float32, device="cuda")
        for name, trav in [t for t in TRAVERSALS if t[0] in traversals]:
            p = z.RenderParams(1, 1, 1, 1, traversal=trav)
            a_all, h_all, occ = time_kernels(ctx, p, rays_dev, n, tm, warm, reps)
            sub = torch.from_numpy(rays[occ]).cuda()
            m = int(occ.sum())
            tm_sub = None if tm is None else tm[:m].contiguous()
            a_occ, h_occ, occ2 = time_kernels(ctx, p, sub, m, tm_sub, warm, reps) if m else (None, None, occ[:0])
            assert occ2.all()
            rec["kernels"].append({"t_max": label, "traversal": name, "occluded": m, "anyhit_ms": a_all,
                                   "closest_hit_ms": h_all, "occluded_subset": {"rays": m, "anyhit_ms": a_occ,
                                                                                 "closest_hit_ms": h_occ}})
            print(json.dumps(rec["kernels"][-1]), flush=True)
    # wall time per batch: a resident context against the one-shot call (FAST)
    p = z.RenderParams(1, 1, 1, 1)
    t = torch.zeros(n, dtype=torch.float32, device="cuda")
    prim = torch.zeros(n, dtype=torch.int32, device="cuda")
    res, one = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        ctx.trace(p, rays_dev.data_ptr(), n, t.data_ptr(), prim.data_ptr())
        ctx.sync()
        dt = time.perf_counter() - t0
        if i >= warm:
            res.append(dt * 1e3)
    for i in range(1 + min(reps, 5)):
        t0 = time.perf_counter()
        t1, p1 = z.trace(scene, p, rays[:, :3], rays[:, 3:])
        dt = time.perf_counter() - t0
        if i >= 1:
            one.append(dt * 1e3)
    assert np.array_equal(t1.view(np.uint32), t.cpu().numpy().view(np.uint32)) and np.array_equal(p1, prim.cpu().numpy())
    rec["resident_vs_one_shot"] = {"traversal": "fast", "rays": n, "resident_wall_ms": spread(res),
                                   "one_shot_wall_ms": spread(one)}
    print(json.dumps(rec["resident_vs_one_shot"]), flush=True)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[2])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--traversals", nargs="+", default=[t[0] for t in TRAVERSALS])
    ap.add_argument("--out", default=os.path.join("profiles", "r15", "queries"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for k in a.scenes:
        rec = probe_scene(k, a.size, a.rays, a.warmup, a.repeats, a.traversals)
        rec["build_id"] = z.build_id()
        rec["device"] = torch.cuda.get_device_name(0)
        with open(os.path.join(a.out, f"ao_scene{k}.json"), "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

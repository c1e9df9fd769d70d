"""Measure the fused ambient-occlusion kernel (zrt_ctx_ao) against the unfused path on the
same rays (GPU box).

Workload: a size x size feature buffer of the scene (zrt_ctx_features), n AO rays per pixel,
radius +inf and 0.25 x the extent of the hit points.  Fused: zrt_ctx_ao, kernel time
zrt_ctx_ao_ms, wall time around call + zrt_ctx_sync.  Unfused: the rays built in torch
(P = o + dir t, d = N + r, packed to n x 6 f32; r, the unit vectors of the pixels' streams,
is made once on the host and not timed: the fused kernel pays for its RNG, this path does
not), zrt_ctx_occluded on them (kernel time zrt_ctx_query_ms: the any-hit kernel alone, the
yardstick), and the per-pixel reduction in torch; wall time around all three.  The host's
sin / cos are not the device's bit for bit, so the two paths' counts are compared and the
pixels that differ are reported, not asserted.  Every figure is min / median / max over
the repeats after warm-up launches.  Writes <out>/ao_scene<k>.json.  zrt_ctx_ao_ms is the
fused kernel alone: with a sample count that does not divide 64 the call also zeroes a count
plane before it and folds the plane in after it (ao_finish_kernel), which only the wall
time covers.

    python tools/ao_probe.py [--scenes 2] [--samples 1 16] [--traversals fast binary] [--size 1024] [--out profiles/r16/ao]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import zraytrace_amd as z

F = np.float32
U = np.uint64
TRAVERSALS = (("fast", z.ZRT_TRAVERSAL_FAST), ("binary", z.ZRT_TRAVERSAL_BINARY), ("reference", z.ZRT_TRAVERSAL_REFERENCE))


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "n": len(xs)}


def _splitmix(s):
    s = s + U(0x9E3779B97F4A7C15)
    x = s
    x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return s, x ^ (x >> U(31))


def _rotl(x, k):
    return (x << U(k)) | (x >> U(64 - k))


def unit_vectors(keys):
    """randomUnitVector of DefaultPrng.init(key) (Xoroshiro128+) per key, in numpy (sin / cos: numpy's)."""
    with np.errstate(over="ignore"):
        g, s0 = _splitmix(keys)
        g, s1 = _splitmix(g)
        draws = []
        for _ in range(3):
            draws.append(s0 + s1)
            b = s1 ^ s0
            s0, s1 = _rotl(s0, 55) ^ b ^ (b << U(14)), _rotl(b, 36)
    fl = lambda r: ((((r & U(0xFFFFFFFF)) >> U(9)) | U(0x7F << 23)).astype(np.uint32).view(F) - F(1))
    r1, r2 = fl(draws[0]), fl(draws[1])
    rr = np.sqrt(F(1) - r1 * r1)
    a = F(2 * np.pi) * r2
    z_ = np.where((draws[2] & U(1)) != 0, r1, -r1)
    return np.stack([np.cos(a) * rr, np.sin(a) * rr, z_], -1).astype(F)


def probe_scene(index, size, samples, warm, reps, traversals, prologue=False):
    scene = z.load_scene(index)
    cam = scene.camera
    ctx = z.RenderContext(scene, z.RenderParams(size, size, 1, 1))
    p0 = z.RenderParams(size, size, 1, 1)
    feat = torch.zeros(size * size * 8, dtype=torch.float32, device="cuda")
    ctx.features(cam, p0, feat.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()
    f = feat.view(size, size, 8)
    v3 = lambda v: torch.tensor([v.x, v.y, v.z], dtype=torch.float32, device="cuda")
    o, llc, hor, ver = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical)
    u = (torch.arange(size, device="cuda", dtype=torch.float32) / size)[None, :, None]
    v = (torch.arange(size, device="cuda", dtype=torch.float32) / size)[:, None, None]
    e = ((llc + hor * u) + ver * v) - o
    dirs = e / torch.sqrt((e * e).sum(-1, keepdim=True))
    hit = f[..., 7].view(torch.int32) != 0
    hit_idx = torch.nonzero(hit.reshape(-1)).reshape(-1)
    pos_all = (o + dirs * f[..., 3:4])[hit]
    extent = float((pos_all.max(0).values - pos_all.min(0).values).max())
    pix = hit_idx.cpu().numpy().astype(U)
    rec = {"scene": index, "n_prims": scene.n_prims, "feature_size": size, "hit_pixels": int(len(pix)),
           "extent": extent, "warmup": warm, "repeats": reps, "runs": []}
    clear = torch.zeros(size * size, dtype=torch.int32, device="cuda")
    plane = torch.zeros(size * size, dtype=torch.float32, device="cuda")
    for n in samples:
        keys = ((pix[:, None] << U(16)) | np.arange(n, dtype=U)[None, :]) + U((42 * 0x9E3779B97F4A7C15) % (1 << 64))
        r_dev = torch.from_numpy(unit_vectors(keys.reshape(-1)).reshape(len(pix), n, 3)).cuda()
        m = len(pix) * n
        out = torch.zeros(m, dtype=torch.uint8, device="cuda")
        radii = [("inf", float("inf")), ("0.25 extent", 0.25 * extent)]
        if prologue:  # a radius no box passes: what the kernels cost before and around the traversal
            radii.append(("0.0011 (no traversal)", 0.0011))
        for label, radius in radii:
            tm = None if radius == float("inf") else torch.full((m,), radius, dtype=torch.float32, device="cuda")
            for name, trav in [t for t in TRAVERSALS if t[0] in traversals]:
                p = z.RenderParams(size, size, 1, 1, traversal=trav)
                ao = z.ao_settings(n, radius)
                plan = z.debug_ao_plan(p, ao, torch.cuda.get_device_properties(0).multi_processor_count)
                fused_ms, fused_wall, any_ms, unfused_wall = [], [], [], []
                for i in range(warm + reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ctx.ao(cam, p, ao, feat.data_ptr(), clear.data_ptr(), plane.data_ptr())
                    ctx.sync()
                    w_f = (time.perf_counter() - t0) * 1e3
                    k_f = ctx.ao_ms()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fh = f.reshape(-1, 8)[hit_idx]
                    P = (o + dirs.reshape(-1, 3)[hit_idx] * fh[:, 3:4])[:, None, :].expand(-1, n, -1)
                    d = fh[:, None, 0:3] + r_dev
                    rays = torch.cat([P, d], -1).reshape(-1, 6).contiguous()
                    torch.cuda.synchronize()
                    ctx.occluded(p, rays.data_ptr(), tm.data_ptr() if tm is not None else 0, m, out.data_ptr())
                    ctx.sync()
                    counts = n - out.view(-1, n).sum(1, dtype=torch.int32)
                    torch.cuda.synchronize()
                    w_u = (time.perf_counter() - t0) * 1e3
                    k_u = ctx.query_ms()
                    del rays
                    if i >= warm:
                        fused_ms.append(k_f)
                        fused_wall.append(w_f)
                        any_ms.append(k_u)
                        unfused_wall.append(w_u)
                got = clear[hit_idx]
                run = {"samples": n, "radius": label, "traversal": name, "rays": m, "plan": plan,
                       "occluded_share": float(1.0 - got.sum().item() / m),
                       "pixels_differing_from_unfused": int((got != counts).sum().item()),
                       "fused_kernel_ms": spread(fused_ms), "anyhit_kernel_ms": spread(any_ms),
                       "fused_wall_ms": spread(fused_wall), "unfused_wall_ms": spread(unfused_wall)}
                run["fused_over_anyhit"] = run["fused_kernel_ms"]["median"] / run["anyhit_kernel_ms"]["median"]
                rec["runs"].append(run)
                print(json.dumps(run), flush=True)
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[2])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--traversals", nargs="+", default=["fast", "binary"])
    ap.add_argument("--prologue", action="store_true", help="also a radius of 0.0011: the kernels without traversal")
    ap.add_argument("--out", default=os.path.join("profiles", "r16", "ao"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for k in a.scenes:
        rec = probe_scene(k, a.size, a.samples, a.warmup, a.repeats, a.traversals, a.prologue)
        rec["build_id"] = z.build_id()
        rec["device"] = torch.cuda.get_device_name(0)
        with open(os.path.join(a.out, f"ao_scene{k}.json"), "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

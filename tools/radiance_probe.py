"""Measure the radiance query (zrt_ctx_radiance) against the render of the same frame (GPU box).

Workload: the size x size pixel-centre rays of the scene's camera (u = x / size, v = y / size,
as zrt_ctx_features builds them), n samples per ray at max_depth, sample_chunk 32, in three
ray orders - the render's 8 x 8 tile order, row-major, and randomly permuted - on each
traversal.  Per run: kernel_ms of zrt_ctx_radiance_info (the events around the call's kernels:
radiance_kernel and the folds of radiance_finish_kernel) and Mrays/s from its ray counter.
Beside them the render's kernel time (zrt_ctx_last_kernel_ms) for the same frame, samples and
depth on the same library: its rays are jittered inside their pixels where the query's go
through the pixel corners' lattice, so the two trace the same scene at the same density, not
the same paths; Mrays/s compares them per ray.  Every figure is min / median / max over the
repeats after warm-up launches.  Writes <out>/radiance_scene<k>.json.

    python tools/radiance_probe.py [--scenes 2] [--size 1024] [--samples 32] [--depth 20] [--traversals fast binary] [--out profiles/r17/radiance]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

import zraytrace_amd as z

TRAVERSALS = (("fast", z.ZRT_TRAVERSAL_FAST), ("binary", z.ZRT_TRAVERSAL_BINARY), ("reference", z.ZRT_TRAVERSAL_REFERENCE))


def spread(xs):
    xs = sorted(xs)
    return {"min": xs[0], "median": xs[len(xs) // 2], "max": xs[-1], "n": len(xs)}


def pixel_rays(cam, size):
    """float32[size * size, 6] on the device, row-major from the bottom row."""
    v3 = lambda v: torch.tensor([v.x, v.y, v.z], dtype=torch.float32, device="cuda")
    o, llc, hor, ver = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical)
    u = (torch.arange(size, device="cuda", dtype=torch.float32) / size)[None, :, None]
    v = (torch.arange(size, device="cuda", dtype=torch.float32) / size)[:, None, None]
    d = (((llc + hor * u) + ver * v) - o).reshape(-1, 3)
    return torch.cat([o.expand(len(d), 3), d], 1).contiguous()


def orders(size):
    """Permutations of the row-major ray index: name -> int64[size * size]."""
    idx = torch.arange(size * size, device="cuda").view(size, size)
    t = size // 8
    tiles = idx.view(t, 8, t, 8).permute(0, 2, 1, 3).reshape(-1)  # tile rows, tiles, the tile's 8 x 8 pixels
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    return {"tiles 8x8": tiles, "row-major": idx.reshape(-1), "random": torch.randperm(size * size, device="cuda", generator=g)}


def probe_scene(index, size, samples, depth, warm, reps, traversals):
    scene = z.load_scene(index)
    cam = scene.camera
    ctx = z.RenderContext(scene, z.RenderParams(size, size, samples, depth))
    base = pixel_rays(cam, size)
    n = size * size
    sums = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rec = {"scene": index, "n_prims": scene.n_prims, "size": size, "samples": samples, "max_depth": depth,
           "warmup": warm, "repeats": reps, "runs": []}
    for name, trav in [t for t in TRAVERSALS if t[0] in traversals]:
        p = z.RenderParams(size, size, samples, depth, traversal=trav)
        tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
        render_ms = []
        for i in range(warm + reps):
            ctx.render_tiles(cam, p, tiles.data_ptr())
            ctx.sync()
            if i >= warm:
                render_ms.append(ctx.kernel_ms())
        st = ctx.stats()
        render = {"traversal": name, "kernel_ms": spread(render_ms), "rays": st["rays_processed"]}
        render["mrays_per_s"] = render["rays"] / render["kernel_ms"]["median"] / 1e3
        rq = z.radiance_settings(samples)
        plan = z.debug_radiance_plan(p, rq, n, cus)
        for label, perm in orders(size).items():
            rays = base[perm].contiguous()
            torch.cuda.synchronize()
            ms = []
            for i in range(warm + reps):
                ctx.radiance(p, rq, rays.data_ptr(), n, sums.data_ptr(), rgb.data_ptr())
                ctx.sync()
                info = ctx.radiance_info()
                if i >= warm:
                    ms.append(info["kernel_ms"])
            run = {"traversal": name, "order": label, "kernel_ms": spread(ms), "rays": info["rays"],
                   "reflections": info["reflections"], "plan": plan, "launch": ctx.debug_radiance(), "render": render}
            run["mrays_per_s"] = run["rays"] / run["kernel_ms"]["median"] / 1e3
            run["radiance_over_render_ms"] = run["kernel_ms"]["median"] / render["kernel_ms"]["median"]
            run["radiance_over_render_per_ray"] = render["mrays_per_s"] / run["mrays_per_s"]
            run["mean_rgb"] = [float(x) for x in rgb.mean(0).cpu()]
            rec["runs"].append(run)
            print(json.dumps(run), flush=True)
            del rays
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[2])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--depth", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--traversals", nargs="+", default=["fast", "binary"])
    ap.add_argument("--out", default=os.path.join("profiles", "r17", "radiance"))
    a = ap.parse_args()
    if a.size % 8:
        ap.error("--size must be a multiple of 8 (the tile order)")
    os.makedirs(a.out, exist_ok=True)
    for k in a.scenes:
        rec = probe_scene(k, a.size, a.samples, a.depth, a.warmup, a.repeats, a.traversals)
        rec["build_id"] = z.build_id()
        rec["device"] = torch.cuda.get_device_name(0)
        with open(os.path.join(a.out, f"radiance_scene{k}.json"), "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

"""Measure the camera query (zrt_ctx_camera) against the radiance query and the render (GPU box).

Workload: the size x size frame of the scene's camera, n samples per pixel at max_depth,
sample_chunk 32, on each traversal:
  camera    zrt_ctx_camera over the whole frame through the pinhole (the scene camera's own
            plane), a thin lens (aperture and focal distance below) and the equirectangular
            model, each from the camera's pose (zrt_lens_from_camera);
  radiance  zrt_ctx_radiance over the frame's pixel-centre rays in 8 x 8 tile order
            (tools/radiance_probe.py's "tiles 8x8"), on this library;
  render    zrt_ctx_render_tiles of the same frame.
Per run: kernel_ms between the events around the call's kernels (min / median / max over the
repeats after warm-up launches) and Mrays/s from the call's ray counter.  The three trace
the same scene at the same density, not the same paths.  Writes <out>/camera_scene<k>.json.

    python tools/camera_probe.py [--scenes 2] [--size 1024] [--samples 32] [--depth 20] [--traversals fast binary] [--out profiles/r18/camera]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

import zraytrace_amd as z

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from radiance_probe import TRAVERSALS, orders, pixel_rays, spread  # noqa: E402


def probe_scene(index, size, samples, depth, warm, reps, traversals, aperture, focus):
    scene = z.load_scene(index)
    cam = scene.camera
    ctx = z.RenderContext(scene, z.RenderParams(size, size, samples, depth))
    n = size * size
    sums = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    rays = pixel_rays(cam, size)[orders(size)["tiles 8x8"]].contiguous()
    torch.cuda.synchronize()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lenses = {"pinhole": z.lens_from_camera(z.ZRT_LENS_PINHOLE, cam),
              "thin": z.lens_from_camera(z.ZRT_LENS_THIN, cam, aperture=aperture, focus_dist=focus),
              "equirect": z.lens_from_camera(z.ZRT_LENS_EQUIRECT, cam)}
    q = z.camera_query(0, 0, size, size, samples)
    rec = {"scene": index, "n_prims": scene.n_prims, "size": size, "samples": samples, "max_depth": depth,
           "warmup": warm, "repeats": reps, "aperture": aperture, "focus_dist": focus, "runs": []}
    for name, trav in [t for t in TRAVERSALS if t[0] in traversals]:
        p = z.RenderParams(size, size, samples, depth, traversal=trav)
        tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")

        def timed(what, launch, info):
            ms = []
            for i in range(warm + reps):
                launch()
                ctx.sync()
                got = info()
                if i >= warm:
                    ms.append(got["kernel_ms"])
            run = {"traversal": name, "what": what, "kernel_ms": spread(ms), "rays": got["rays"]}
            run["mrays_per_s"] = run["rays"] / run["kernel_ms"]["median"] / 1e3
            return run

        def render_info():
            return {"kernel_ms": ctx.kernel_ms(), "rays": ctx.stats()["rays_processed"]}

        runs = [timed("render", lambda: ctx.render_tiles(cam, p, tiles.data_ptr()), render_info)]
        rq = z.radiance_settings(samples)
        runs.append(timed("radiance, tiles 8x8",
                          lambda: ctx.radiance(p, rq, rays.data_ptr(), n, sums.data_ptr(), rgb.data_ptr()), ctx.radiance_info))
        for model, lens in lenses.items():
            run = timed("camera, " + model, lambda: ctx.camera(p, lens, q, sums.data_ptr(), rgb.data_ptr()), ctx.camera_info)
            run["mean_rgb"] = [float(x) for x in rgb.mean(0).cpu()]
            run["launch"] = ctx.debug_radiance()
            runs.append(run)
        by = {r["what"]: r for r in runs}
        for r in runs:
            r["over_radiance_ms"] = r["kernel_ms"]["median"] / by["radiance, tiles 8x8"]["kernel_ms"]["median"]
            r["over_pinhole_ms"] = r["kernel_ms"]["median"] / by["camera, pinhole"]["kernel_ms"]["median"]
            r["over_render_per_ray"] = by["render"]["mrays_per_s"] / r["mrays_per_s"]
            print(json.dumps(r), flush=True)
        rec["plan"] = z.debug_camera_plan(p, q, cus)
        rec["runs"] += runs
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
    ap.add_argument("--aperture", type=float, default=0.02)
    ap.add_argument("--focus", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join("profiles", "r18", "camera"))
    a = ap.parse_args()
    if a.size % 8:
        ap.error("--size must be a multiple of 8 (the tile order)")
    os.makedirs(a.out, exist_ok=True)
    for k in a.scenes:
        rec = probe_scene(k, a.size, a.samples, a.depth, a.warmup, a.repeats, a.traversals, a.aperture, a.focus)
        rec["build_id"] = z.build_id()
        rec["device"] = torch.cuda.get_device_name(0)
        with open(os.path.join(a.out, f"camera_scene{k}.json"), "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()

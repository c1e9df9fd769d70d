"""Regenerate tests/golden/sphere_tiles_scene2_64x64x128.npz: the oracle's whole frames and
Progress counters of scene 2 at 64 x 64 x 128 spp (chunk 32, seed 7 + depth) for depths 1, 2,
20 and both generators - tests/test_gpu_sphere_tiles.py's scheduled frames, which take the
oracle half a minute each.  usage: python tests/golden/make_sphere_tiles_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import zraytrace_amd as z  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

COUNTERS = ("recursion_depth_hits", "reflections", "background_hits", "rays_processed", "pixels_processed",
            "samples_processed")


def main():
    s = z.load_scene(2)
    out = {}
    for depth in (1, 2, 20):
        for prng in (z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256):
            p = z.RenderParams(64, 64, 128, depth, prng=prng, seed=7 + depth, sample_chunk=32)
            img, st = O.render(s.view, s.camera, p)
            out[f"frame_d{depth}_p{prng}"] = img
            out[f"counters_d{depth}_p{prng}"] = np.array([st[k] for k in COUNTERS], np.uint64)
    np.savez_compressed(os.path.join(HERE, "sphere_tiles_scene2_64x64x128.npz"), **out)


if __name__ == "__main__":
    main()

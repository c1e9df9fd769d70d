"""CPU tests of the radiance-query reference (tests/radiance_ref.py): the 1 x 1 form is the
oracle's own pixel, the seed shift is exact, and the sums composed per sample have the
oracle's mean.  No kernel is launched."""
import functools

import numpy as np
import pytest

import radiance_ref as R
import shading_scenes as S
import zraytrace_amd as z
from oracle import oracle_py as O

F = np.float32
SCENES = ("bubbles", "wraps", "glass-inside")
PRNGS = [z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256]
CASES = [(5, 2, 6), (3, 0, 1), (1, 0, 0)]  # (samples, sample_chunk, max_depth)
N_RAYS = 48


@functools.lru_cache(maxsize=None)
def rays():
    return R.scattered_rays(N_RAYS, seed=5)


def params(prng, chunk, depth, seed=42):
    return z.RenderParams(1, 1, 1, depth, seed=seed, prng=prng, sample_chunk=chunk)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("prng", PRNGS, ids=["xoroshiro", "xoshiro"])
@pytest.mark.parametrize("spp,chunk,depth", CASES)
def test_two_forms_agree(name, prng, spp, chunk, depth):
    """Ray R as a 1 x 1 frame under the shifted seed is pixel R of an 8 x 8 frame of the
    degenerate camera under the call's seed: colours bitwise, on every ray."""
    _, view, _ = S.get(name)
    o, t = rays()
    p = params(prng, chunk, depth)
    rgb, info = R.expected(O, view, p, o, t, spp)
    for i in range(N_RAYS):
        want, _ = R.frame_form(O, view, p, o[i], t[i], spp, i)
        assert R.same_bits(rgb[i], want).all(), f"ray {i}: {rgb[i]} != {want}"
    assert info["samples"] == N_RAYS * spp
    assert info["rays"] == info["samples"] + info["reflections"] - info["recursion_depth_hits"]
    if depth == 0:
        assert not rgb.any() and info["recursion_depth_hits"] == info["samples"] and info["rays"] == 0
    if depth == 6:  # the rays are worth comparing: most of them carry colour
        assert int((rgb != 0).any(1).sum()) >= N_RAYS * 3 // 4


@pytest.mark.parametrize("prng", PRNGS, ids=["xoroshiro", "xoshiro"])
def test_seed_identity_at_a_large_ray_index(prng):
    ray = (1 << 40) + 5
    for seed in (0, 42, (1 << 64) - 3):
        for s in (0, 1, 65535):
            shifted = R.shifted_seed(seed, ray)
            assert R.key_of(0, s, shifted) == R.key_of(ray, s, seed)
            assert R.key_of(0, 0, R.shifted_seed(seed, ray, s)) == R.key_of(ray, s, seed)
    # and through the oracle: sample s of the 1 x 1 frame is the one-sample frame keyed onto (ray, s)
    _, view, _ = S.get("wraps")
    o, t = rays()
    p = params(prng, 0, 6)
    rgb, _ = R.expected(O, view, p, o[:8], t[:8], 1, first_ray=ray)
    cols = R.sample_colors(O, view, p, o[:8], t[:8], 0, 1, first_ray=ray)
    assert R.same_bits(rgb, cols[:, 0]).all()
    other, _ = R.expected(O, view, p, o[:8], t[:8], 1, first_ray=ray + 1)
    assert not R.same_bits(rgb, other).all(), "the ray index does not reach the stream"


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("spp,chunk", [(5, 2), (9, 4), (4, 4), (3, 0)])
def test_composed_sums_have_the_oracles_mean(name, spp, chunk):
    _, view, _ = S.get(name)
    o, t = rays()
    p = params(z.ZRT_PRNG_XOROSHIRO128, chunk, 6)
    rgb, _ = R.expected(O, view, p, o[:16], t[:16], spp)
    sums = R.chunk_sums(R.sample_colors(O, view, p, o[:16], t[:16], 0, spp), chunk)
    assert R.same_bits(R.mean_of(sums, spp), rgb).all()
    assert not sums[:, 3].any()


def test_chunk_sums_continue_across_calls():
    """Accumulating [0, 8) then [8, 16) at chunk 4 or 8 is the one sum over [0, 16)."""
    rng = np.random.default_rng(1)
    cols = rng.random((7, 16, 3), dtype=F)
    for c in (4, 8):
        whole = R.chunk_sums(cols, c)
        for cut in (8, 4) if c == 4 else (8,):
            part = R.chunk_sums(cols[:, cut:], c, R.chunk_sums(cols[:, :cut], c))
            assert R.same_bits(part, whole).all()

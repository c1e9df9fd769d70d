"""CPU tests of how zrt_ctx_radiance launches and what it refuses (zrt_debug_radiance_plan:
no device; the launch path calls the same function), and of the equirectangular ray
generator.  No kernel is launched."""
import math

import numpy as np
import pytest

import zraytrace_amd as z

F = np.float32
GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1


def params(chunk=0, seed=42, **kw):
    return z.RenderParams(1, 1, 1, 8, seed=seed, sample_chunk=chunk, **kw)


def plan(n, n_samples, chunk=0, cu=256, cap=0, **rq):
    return z.debug_radiance_plan(params(chunk), z.radiance_settings(n_samples, **rq), n, cu, cap)


def test_chunking_and_the_ragged_last_chunk():
    for n_samples, chunk, chunks, last in [(9, 4, 3, 1), (8, 4, 2, 4), (1, 4, 1, 1), (33, 0, 2, 1), (32, 0, 1, 32),
                                           (5, 9, 1, 5), (65536, 1, 65536, 1), (9, (1 << 32) - 1, 1, 9),
                                           (65536, 1 << 31, 1, 65536)]:
        p = plan(100, n_samples, chunk)
        assert (p["chunk"], p["call_chunks"], p["last_chunk"]) == (chunk or 32, chunks, last), (n_samples, chunk)
        assert p["items"] == 100 * chunks
        assert p["chunks_per_round"] * (p["rounds"] - 1) < chunks <= p["chunks_per_round"] * p["rounds"]


def test_items_past_32_bits():
    n = (1 << 32) - 1
    p = plan(n, 4096, 2)
    assert p["call_chunks"] == 2048 and p["items"] == n * 2048 > 1 << 32
    # one chunk of every ray is 64 GiB: past the default cap, so one chunk per round
    assert p["chunks_per_round"] == 1 and p["rounds"] == 2048 and p["partial_bytes"] == n * 16
    assert p["grid"] == 16 * 256 and p["resident_lanes"] == p["grid"] * 256  # by the CUs, never by the rays


def test_rounds_under_a_small_cap():
    n = 257
    for cap, cpr, rounds in [(n * 16, 1, 3), (n * 16 * 2, 2, 2), (n * 16 * 3 - 1, 2, 2), (n * 16 * 3, 3, 1), (1, 1, 3),
                             (0, 3, 1)]:
        p = plan(n, 9, 4, cap=cap)
        assert (p["chunks_per_round"], p["rounds"]) == (cpr, rounds), cap
        assert p["partial_bytes"] == n * cpr * 16
        assert cap == 0 or p["partial_bytes"] <= max(cap, n * 16)


def test_grid_is_bounded_by_the_cu_count():
    for cu in (1, 256):
        big = plan(1 << 20, 64, 4, cu=cu)
        assert big["grid"] == big["blocks_per_cu"] * cu
        assert big["resident_lanes"] == big["grid"] * 256
        small = plan(65, 3, 4, cu=cu)  # 65 items: one block
        assert small["grid"] == 1
    assert plan(257, 9, 4, cu=256)["grid"] == 4  # ceil(257 * 3 / 256)
    assert plan(257, 9, 4, cu=256, cap=257 * 16)["grid"] == 2  # a round of one chunk: ceil(257 / 256)


def test_key_offset():
    for first_ray, seed in [(0, 42), ((1 << 40) + 5, 42), ((1 << 48) - 7, (1 << 64) - 1)]:
        p = z.debug_radiance_plan(params(seed=seed), z.radiance_settings(1, first_ray=first_ray), 7, 256)
        assert p["key_offset"] == ((first_ray << 16) + seed * GOLDEN) & MASK64


def test_no_rays_is_a_plan_of_nothing():
    p = plan(0, 5, 2)
    assert p["items"] == 0 and p["grid"] == 0 and p["rounds"] == 0 and p["call_chunks"] == 3


@pytest.mark.parametrize("what,kw", [
    ("n_samples == 0", dict(n=4, n_samples=0)),
    ("first_sample + n_samples > 65536", dict(n=4, n_samples=2, first_sample=65535)),
    ("n_samples > 65536", dict(n=4, n_samples=65537)),
    ("first_ray + n > 2^48", dict(n=4, n_samples=1, first_ray=(1 << 48) - 3)),
    ("first_ray > 2^48", dict(n=0, n_samples=1, first_ray=(1 << 48) + 1)),
    ("an unknown flag", dict(n=4, n_samples=1, flags=2)),
    ("accumulate, misaligned first_sample", dict(n=4, n_samples=4, first_sample=6, flags=z.ZRT_RQ_ACCUMULATE, chunk=4)),
    ("accumulate, misaligned at the default chunk", dict(n=4, n_samples=4, first_sample=16, flags=z.ZRT_RQ_ACCUMULATE)),
    ("cu_count == 0", dict(n=4, n_samples=1, cu=0)),
])
def test_refusals(what, kw):
    with pytest.raises(z.ZrtError) as e:
        plan(**kw)
    assert e.value.code == z._ffi.ZRT_E_INVALID, what


def test_refuses_an_unknown_traversal():
    with pytest.raises(z.ZrtError):
        z.debug_radiance_plan(params(traversal=7), z.radiance_settings(1), 4, 256)


def test_what_is_allowed_at_the_edges():
    assert plan(4, 1, first_sample=65535)["call_chunks"] == 1
    assert plan(3, 1, first_ray=(1 << 48) - 3)["items"] == 3
    assert plan(4, 4, 4, first_sample=8, flags=z.ZRT_RQ_ACCUMULATE)["call_chunks"] == 1
    assert plan(4, 4, 4, first_sample=6)["call_chunks"] == 1  # no flag: any first_sample


def test_equirect_4x2():
    o = np.array([1.5, -2.0, 0.25], F)
    r = z.rays_equirect(o, 4, 2)
    assert r.shape == (2, 4, 6) and r.dtype == F
    assert (r[..., :3] == o).all()
    for y in range(2):
        theta = math.pi * (y + 0.5) / 2
        for x in range(4):
            phi = 2 * math.pi * (x + 0.5) / 4
            want = np.array([math.sin(theta) * math.cos(phi), -math.cos(theta), math.sin(theta) * math.sin(phi)]).astype(F)
            assert (r[y, x, 3:].view(np.uint32) == want.view(np.uint32)).all(), (x, y)
    assert (r[0, :, 4] < 0).all() and (r[1, :, 4] > 0).all()  # row 0 is the bottom: it looks down
    with pytest.raises(z.ZrtError):
        z.rays_equirect(o, 0, 2)

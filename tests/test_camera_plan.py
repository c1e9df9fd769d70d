"""CPU tests of how zrt_ctx_camera launches and what it refuses (zrt_debug_camera_plan and
zrt_lens_check: no device; the launch path calls the same functions).  No kernel is launched."""
import math

import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi

GOLDEN = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
POSE = ((0.4, 1.7, -3.6), (0.1, 0.2, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5)


def params(width=24, height=16, chunk=4, seed=42, **kw):
    return z.RenderParams(width, height, 1, 8, seed=seed, sample_chunk=chunk, **kw)


def plan(rect, n_samples=9, width=24, height=16, chunk=4, cu=256, cap=0, first_sample=0, flags=0, **kw):
    return z.debug_camera_plan(params(width, height, chunk, **kw), z.camera_query(*rect, n_samples, first_sample, flags),
                               cu, cap)


def slot_pixels(rect, p):
    """The pixels zrt.h gives the plan's slots, in slot order (None: outside the rectangle)."""
    x0, y0, w, h = rect
    out = []
    for slot in range(p["slots"]):
        t, lane = divmod(slot, 64)
        lx, ly = 8 * (t % p["tiles_w"]) + (lane & 7), 8 * (t // p["tiles_w"]) + (lane >> 3)
        out.append((x0 + lx, y0 + ly) if lx < w and ly < h else None)
    return out


@pytest.mark.parametrize("rect,tiles", [((0, 0, 24, 16), (3, 2)), ((3, 5, 13, 9), (2, 2)), ((23, 15, 1, 1), (1, 1)),
                                        ((0, 0, 8, 8), (1, 1)), ((1, 0, 9, 16), (2, 2)), ((0, 7, 24, 1), (3, 1))])
def test_slots_and_tiles(rect, tiles):
    p = plan(rect)
    assert (p["tiles_w"], p["tiles_h"]) == tiles
    assert p["slots"] == tiles[0] * tiles[1] * 64 and p["pixels"] == rect[2] * rect[3]
    px = slot_pixels(rect, p)
    inside = [q for q in px if q is not None]
    assert len(inside) == len(set(inside)) == p["pixels"]  # every pixel of the rectangle once
    assert set(inside) == {(x, y) for x in range(rect[0], rect[0] + rect[2]) for y in range(rect[1], rect[1] + rect[3])}
    r = p["radiance"]
    assert r["items"] == p["slots"] * r["call_chunks"] and r["items"] % 64 == 0
    assert (r["chunk"], r["call_chunks"], r["last_chunk"]) == (4, 3, 1)
    assert r == z.debug_radiance_plan(params(), z.radiance_settings(9), p["slots"], 256, 0)
    assert r["key_offset"] == (42 * GOLDEN) & MASK64


def test_rounds_and_grid():
    rect = (0, 0, 40, 24)  # 15 tiles: 960 slots, past a block
    p = plan(rect, width=40, height=24)
    assert p["slots"] == 960 and p["radiance"]["grid"] == math.ceil(960 * 3 / 256)
    assert (p["radiance"]["chunks_per_round"], p["radiance"]["rounds"]) == (3, 1)
    for cap, cpr, rounds in [(960 * 16, 1, 3), (960 * 16 * 2, 2, 2), (1, 1, 3)]:
        r = plan(rect, width=40, height=24, cap=cap)["radiance"]
        assert (r["chunks_per_round"], r["rounds"]) == (cpr, rounds)
        assert r["partial_bytes"] == 960 * cpr * 16
    big = plan((0, 0, 65535, 65527), 64, width=65535, height=65535, cu=4)
    assert (big["tiles_w"], big["tiles_h"]) == (8192, 8191) and big["slots"] == 8192 * 8191 * 64 < 1 << 32
    assert big["radiance"]["items"] == big["slots"] * 16 > 1 << 32
    assert big["radiance"]["grid"] == big["radiance"]["blocks_per_cu"] * 4  # by the CUs, never by the pixels


def test_refusals_of_the_query():
    def refused(rect, **kw):
        with pytest.raises(z.ZrtError) as e:
            plan(rect, **kw)
        assert e.value.code == _ffi.ZRT_E_INVALID

    plan((0, 0, 24, 16))
    refused((0, 0, 0, 16))  # an empty rectangle
    refused((0, 0, 24, 0))
    refused((1, 0, 24, 16))  # one that leaves the frame
    refused((0, 1, 24, 16))
    refused((24, 0, 1, 1))
    refused((0, 16, 1, 1))
    refused(((1 << 32) - 1, 0, 2, 1))  # x0 + w wraps
    refused((0, 0, 24, 16), flags=2)  # an unknown flag
    refused((0, 0, 24, 16), flags=3)
    refused((0, 0, 24, 16), n_samples=0)
    refused((0, 0, 24, 16), n_samples=65537)
    refused((0, 0, 24, 16), n_samples=2, first_sample=65535)
    plan((0, 0, 24, 16), n_samples=1, first_sample=65535)
    refused((0, 0, 24, 16), first_sample=2, flags=z.ZRT_CQ_ACCUMULATE)  # not a multiple of the chunk
    plan((0, 0, 24, 16), first_sample=2)
    plan((0, 0, 24, 16), first_sample=8, flags=z.ZRT_CQ_ACCUMULATE)
    refused((0, 0, 24, 16), traversal=9)
    refused((0, 0, 24, 16), prng=7)
    refused((0, 0, 24, 16), cu=0)
    refused((0, 0, 1, 1), width=0)
    refused((0, 0, 1, 1), width=65536, height=1)
    refused((0, 0, 1, 1), width=1, height=65536)
    plan((65534, 0, 1, 1), width=65535, height=1)  # the whole width is addressable: height < width is no condition
    plan((0, 65534, 1, 1), width=1, height=65535)
    # the largest frame has 8192 x 8192 tiles: 2^32 slots do not fit the radiance plan's n
    refused((0, 0, 65535, 65535), width=65535, height=65535)
    plan((0, 0, 65535, 65527), width=65535, height=65535)
    for args in [(None, z.camera_query(0, 0, 1, 1, 1)), (params().abi(), None)]:
        out = _ffi.CameraPlan()
        import ctypes as C
        rc = z.lib().zrt_debug_camera_plan(C.byref(args[0]) if args[0] is not None else None,
                                           C.byref(args[1]) if args[1] is not None else None, 1, 0, C.byref(out))
        assert rc == _ffi.ZRT_E_INVALID


def test_refusals_of_the_lens():
    def refused(lens):
        with pytest.raises(z.ZrtError) as e:
            z.lens_check(lens)
        assert e.value.code == _ffi.ZRT_E_INVALID

    for kind in range(5):
        z.lens_check(z.lens_init(kind, *POSE, aperture=0.2, focus_dist=3.0))
    lens = z.lens_init(z.ZRT_LENS_FISHEYE, *POSE)
    lens.kind = 5
    refused(lens)
    for field in ("origin", "lower_left_corner", "horizontal", "vertical", "axis_u", "axis_v", "axis_w"):
        for comp in "xyz":
            for bad in (float("nan"), float("inf"), -float("inf")):
                lens = z.lens_init(z.ZRT_LENS_THIN, *POSE, aperture=0.2, focus_dist=3.0)
                setattr(getattr(lens, field), comp, bad)
                refused(lens)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        lens = z.lens_init(z.ZRT_LENS_PINHOLE, *POSE)
        lens.half_fov = bad
        refused(lens)
    assert z.lib().zrt_lens_check(None) == _ffi.ZRT_E_INVALID

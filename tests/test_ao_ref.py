"""CPU tests of the ambient-occlusion reference and of the launch plan.

1. tests/ao_ref.py on the scenes tests/test_gpu_ao.py uses: the GPU inputs are not
   vacuous (a share of the rays is occluded, a share gets away, pixels are partly
   occluded, the camera inside the glass sphere sees nothing of the sky).  The counts
   are printed; DESIGN.md §5 "Ambient occlusion" records them.
2. zrt_debug_ao_plan: every refusal of zrt_ctx_ao that needs no device, the bounded grid
   and the reduction kinds.
3. The CLI refuses bad AO settings before it renders anything (no device is touched).
"""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import ao_ref as AO
import shading_scenes as S
import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

F = np.float32
W = H = 24
N = 8


@functools.lru_cache(maxsize=None)
def case(name, radius):
    _, view, cam = S.get(name)
    return AO.AoCase(O, view, cam, W, H, radius=radius)


def tally(name, radius):
    c = case(name, radius)
    occ = c.occluded(0, N)
    partly = int(((occ.sum(1) > 0) & (occ.sum(1) < N)).sum())
    print(f"{name} radius {radius}: {occ.size} AO rays ({len(c.ys)} hit pixels), {int(occ.sum())} occluded, "
          f"{partly} pixels partly occluded")
    return occ, partly


@pytest.mark.parametrize("name", ["wraps", "bubbles"])
def test_reference_inputs_are_not_vacuous(name):
    for radius in (math.inf, 0.75):
        occ, partly = tally(name, radius)
        assert occ.size >= 2000
        assert 0.05 < occ.mean() < 0.90, (name, radius, occ.mean())
        if radius == math.inf:
            assert partly >= 100
    occ_near, _ = tally(name, 0.2)
    assert occ_near.sum() <= tally(name, 0.75)[0].sum() <= tally(name, math.inf)[0].sum()


def test_camera_inside_the_glass_sphere_is_fully_occluded():
    occ, _ = tally("glass-inside", math.inf)
    assert occ.size == W * H * N and occ.all()
    occ, _ = tally("glass-inside", 0.75)
    assert 0.05 < occ.mean() < 0.90


def test_no_ray_is_degenerate_and_directions_are_cosine_sided():
    """N + r never vanishes on these inputs, and lies on N's side (|r| = 1 up to rounding)."""
    c = case("wraps", math.inf)
    for s in range(N):
        d = c.directions(s)
        assert np.isfinite(d).all() and (np.abs(d).max(1) > 0).all()
        assert ((d * c.N).sum(1) > -1e-6).all()


def test_reference_composition():
    """A call's counts: n on a miss, the unoccluded samples on a hit; sample ranges add up;
    accumulation divides by the samples so far; a poisoned pixel stays poisoned."""
    c = case("wraps", math.inf)
    assert c.miss.any() and c.hit.any() and not c.poison.any()
    c16, a16 = c.expected(0, 16)
    lo, _ = c.expected(0, 8)
    hi, _ = c.expected(8, 8)
    assert np.array_equal(lo + hi, c16) and (c16[c.miss] == 16).all() and (a16[c.miss] == 1.0).all()
    acc, ao = c.expected(8, 8, prior=lo)
    assert np.array_equal(acc, c16) and np.array_equal(ao.view(np.uint32), a16.view(np.uint32))
    assert np.array_equal(a16, c16.astype(F) / F(16))
    f = c.features.copy()
    y, x = int(c.ys[0]), int(c.xs[0])
    f[y, x, 1] = np.nan
    p = AO.AoCase(O, c.view, c.camera, W, H, features=f)
    clear, ao = p.expected(0, 4)
    assert clear[y, x] == AO.POISON and np.isnan(ao[y, x]) and np.isfinite(np.delete(ao.ravel(), y * W + x)).all()
    clear2, ao2 = p.expected(4, 4, prior=clear)
    assert clear2[y, x] == AO.POISON and np.isnan(ao2[y, x])


def test_key_is_the_counter_modes():
    assert AO.key_of(3, 2, 24, 5, 0) == ((2 * 24 + 3) << 16) | 5
    assert AO.key_of(0, 0, 24, 0, 42) == (42 * 0x9E3779B97F4A7C15) % (1 << 64)


# ---- the launch plan (no device) ---------------------------------------------------------

def plan(w=64, h=64, n=8, first=0, radius=math.inf, flags=0, cu=256, **kw):
    return z.debug_ao_plan(z.RenderParams(w, h, 1, 1, **kw), z.ao_settings(n, radius, first, flags), cu)


def test_plan_refusals():
    assert plan()["rays"] == 64 * 64 * 8
    for kw in (dict(n=0), dict(n=1025), dict(first=65536 - 7, n=8), dict(first=65536, n=1), dict(radius=math.nan),
               dict(radius=0.001), dict(radius=0.0), dict(radius=-1.0), dict(radius=-math.inf), dict(flags=2),
               dict(flags=0x80000001), dict(w=16, h=24), dict(w=0), dict(traversal=3), dict(prng=2), dict(cu=0)):
        with pytest.raises(z.ZrtError) as e:
            plan(**kw)
        assert e.value.code == _ffi.ZRT_E_INVALID, kw
    # the edges that are allowed
    plan(n=1024, first=65536 - 1024)
    plan(n=1, first=65535)
    plan(radius=float(np.nextafter(F(0.001), F(1))))
    plan(flags=_ffi.ZRT_AO_ACCUMULATE)
    plan(w=24, h=16)


def test_plan_counts_rays_in_64_bits_and_bounds_the_grid():
    p = plan(24, 24, 8)
    assert p["pixel_slots"] == 9 * 64 and p["rays"] == 9 * 64 * 8 and p["groups"] == 18
    assert p["grid"] == 18 and p["resident_lanes"] == 18 * 256  # a frame smaller than the grid
    p = plan(20, 20, 3)
    assert p["rays"] == 9 * 64 * 3 and p["groups"] == 7  # 1728 rays: the last group is ragged
    big = plan(1024, 1024, 16)
    assert big["rays"] == 1 << 24 and big["groups"] == 1 << 16
    assert big["grid"] == big["blocks_per_cu"] * 256 and big["resident_lanes"] == big["grid"] * 256
    assert big["ovf_row_bytes"] == big["resident_lanes"] * 4
    # once the frame exceeds the grid, the resident lanes and the rows no longer grow with it
    for w, h, n in ((2048, 2048, 1), (2048, 2048, 16), (4096, 4096, 1024), (65535, 65535, 1024), (1024, 512, 100)):
        q = plan(w, h, n)
        assert (q["grid"], q["resident_lanes"], q["ovf_row_bytes"]) == \
               (big["grid"], big["resident_lanes"], big["ovf_row_bytes"]), (w, h, n)
        assert q["rays"] == ((w + 7) // 8) * ((h + 7) // 8) * 64 * n and q["groups"] == (q["rays"] + 255) // 256
    assert plan(65535, 65535, 1024)["rays"] == 1 << 42  # far past 32 bits
    assert plan(1024, 1024, 16, cu=64)["grid"] == big["blocks_per_cu"] * 64


def test_plan_reduction_kinds():
    for n in (1, 2, 4, 8, 16, 32, 64):
        p = plan(n=n)
        assert p["reduction"] == _ffi.ZRT_AO_REDUCE_WAVE and p["plane_bytes"] == 0, n
    for n in (3, 5, 48, 65, 100, 128, 1024):
        p = plan(40, 24, n)
        assert p["reduction"] == _ffi.ZRT_AO_REDUCE_ATOMIC and p["plane_bytes"] == 40 * 24 * 4, n


# ---- the CLI's refusals (before any device work) ------------------------------------------

@pytest.mark.parametrize("env", [dict(ZRT_AO_OUT="ao.png"), dict(ZRT_AO_SAMPLES="4"), dict(ZRT_AO_RADIUS="1"),
                                 dict(ZRT_AO_SAMPLES="0", ZRT_AO_OUT="ao.png"),
                                 dict(ZRT_AO_SAMPLES="1025", ZRT_AO_OUT="ao.png"),
                                 dict(ZRT_AO_SAMPLES="4x", ZRT_AO_OUT="ao.png"),
                                 dict(ZRT_AO_SAMPLES="4", ZRT_AO_RADIUS="0.0005", ZRT_AO_OUT="ao.png"),
                                 dict(ZRT_AO_SAMPLES="4", ZRT_AO_RADIUS="abc", ZRT_AO_OUT="ao.png")],
                         ids=["out-alone", "samples-alone", "radius-alone", "zero", "too-many", "not-a-number",
                              "radius-too-small", "radius-not-a-number"])
def test_cli_refuses_bad_ao_settings_before_rendering(env, tmp_path):
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    e = {k: v for k, v in os.environ.items() if not k.startswith("ZRT_AO_")}
    e.update({k: str(tmp_path / v) if k == "ZRT_AO_OUT" else v for k, v in env.items()})
    r = subprocess.run([exe, "32", "32", "2", "5", "2", str(tmp_path / "frame.png")], env=e, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode != 0 and "ZRT_AO_" in r.stderr and "Raytrace start" not in r.stderr
    assert not (tmp_path / "frame.png").exists() and not (tmp_path / "ao.png").exists()

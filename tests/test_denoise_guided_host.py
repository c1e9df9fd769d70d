"""Host-side tests of the variance plane and the variance-guided filter (no GPU): the new
entry points and their ctypes signatures, zrt_debug_variance_plan against the numpy f32
expressions, every refusal that needs no device, and the properties of the numpy
restatements (tests/denoise_guided_ref.py) that the GPU tests compare the kernels against."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi

import denoise_guided_ref as G
import denoise_ref as R
import shading_scenes as S

F = np.float32
NEW = ["zrt_ctx_accum_variance", "zrt_ctx_assemble_plane", "zrt_debug_variance_plan", "zrt_denoise_guided_defaults",
       "zrt_ctx_denoise_guided", "zrt_render_denoised_guided"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the interface ----------------------------------------------------------------------

def test_new_symbols_are_exported_and_bound():
    src = open(os.path.join(z.REPO, "include", "zrt.h")).read()
    declared = set(re.findall(r"\b(zrt_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    table = {name for name, _, _ in _ffi.SIGNATURES}
    for name in NEW:
        assert name in declared and name in table, name
        assert getattr(z.lib(), name).argtypes is not None
    assert declared - {"zrt_pass_fn", "zrt_level_fn"} <= table  # the table still covers the header
    assert "#define ZRT_ABI_VERSION 2" in src and z.lib().zrt_abi_version() == 2
    assert "ZRT_DN_DEMODULATE = 1u" in src and z.ZRT_DN_DEMODULATE == 1
    assert C.sizeof(_ffi.VariancePlan) == 16


def test_guided_defaults_are_the_probes_winner():
    d, flags = z.denoise_guided_defaults()
    with open(os.path.join(z.REPO, "profiles", "r11", "guided", "defaults.json")) as f:
        rec = json.load(f)
    assert d.iterations == 5 == rec["winner"]["iterations"]
    for k in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        v = getattr(d, k)
        assert math.isfinite(v) and v >= 0.0 and v == rec["winner"][k], k
    assert flags == rec["winner"]["flags"] and flags in (0, z.ZRT_DN_DEMODULATE)
    assert list(d.reserved) == [0, 0, 0]


# ---- zrt_debug_variance_plan --------------------------------------------------------------

@pytest.mark.parametrize("c", [1, 4, 7, 32])
@pytest.mark.parametrize("k", [2, 3, 8, 2048])
def test_variance_plan_equals_the_f32_expressions(c, k):
    """(32 x 2048 = 65536 samples lie past samples_per_pixel's range: the plan is arithmetic on
    (c, n) and does not bound n by the params.)"""
    p = z.RenderParams(8, 8, 64, 1, sample_chunk=c)
    got = z.debug_variance_plan(p, c * k)
    ik = F(1.0) / F(k)
    sc = F(1.0) / (F(k - 1) * (F(c) * F(c)))
    assert (got["chunk"], got["k"]) == (c, k)
    assert bits(F(got["ik"])) == bits(ik) and bits(F(got["sc"])) == bits(sc)
    assert (bits(F(got["ik"])), bits(F(got["sc"]))) == tuple(bits(x) for x in G.plan(c, k))


def test_variance_plan_default_chunk():
    assert z.debug_variance_plan(z.RenderParams(8, 8, 64, 1), 64)["chunk"] == 32


@pytest.mark.parametrize("c,n,word", [(4, 4, "fewer than two chunks"), (32, 32, "fewer than two chunks"),
                                      (4, 10, "not whole chunks"), (0, 40, "not whole chunks"),
                                      (4, 0, "no samples"), (7, 6, "not whole chunks")])
def test_variance_plan_refusals(c, n, word):
    with pytest.raises(z.ZrtError) as e:
        z.debug_variance_plan(z.RenderParams(8, 8, 64, 1, sample_chunk=c), n)
    assert e.value.code == _ffi.ZRT_E_INVALID and word in str(e.value)
    if "chunk" in word:
        assert "sample_chunk" in str(e.value)


# ---- refusals that need no device -----------------------------------------------------------

def _guided_rc(width=8, height=8, frame=0x1000, feat=0x2000, var=0x3000, out=0x4000, out_var=0x5000, flags=0,
               **fields):
    """zrt_ctx_denoise_guided with no context: what it refuses of its arguments comes first."""
    dn = _ffi.Denoise(iterations=1, sigma_color=1.0, sigma_normal=1.0, sigma_albedo=1.0, sigma_depth=1.0)
    for k, v in fields.items():
        setattr(dn, k, v)
    p = z.RenderParams(width, height, 1, 1).abi()
    rc = z.lib().zrt_ctx_denoise_guided(None, C.byref(p), C.byref(dn), flags, C.c_void_p(frame), C.c_void_p(feat),
                                        C.c_void_p(var), C.c_void_p(out), C.c_void_p(out_var), None)
    return rc, z.lib().zrt_last_error().decode()


@pytest.mark.parametrize("field", ["sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"])
@pytest.mark.parametrize("value", [-1.0, float("nan"), float("inf")])
def test_guided_bad_sigma_is_refused(field, value):
    rc, msg = _guided_rc(**{field: value})
    assert rc == _ffi.ZRT_E_INVALID and field in msg


def test_guided_other_refusals():
    for kw, word in (({"iterations": 9}, "iterations"), ({"width": 8, "height": 9}, "height > width"),
                     ({"out": 0x1000}, "dev_out must not be dev_frame"), ({"feat": 0x2004}, "aligned"),
                     ({"var": None}, "dev_variance is null"), ({"out_var": 0x3000}, "dev_out_variance must not"),
                     ({"flags": 2}, "unknown flag")):
        rc, msg = _guided_rc(**kw)
        assert rc == _ffi.ZRT_E_INVALID and word in msg, (kw, msg)
    # what is valid gets as far as the missing context
    for kw in ({"iterations": 8, "sigma_color": 0.0}, {"iterations": 0, "flags": 1}, {"out_var": None}):
        rc, msg = _guided_rc(**kw)
        assert rc == _ffi.ZRT_E_INVALID and msg == "null argument", (kw, msg)


def test_render_denoised_guided_refuses_before_any_device_work():
    """Bad filters and sample counts the variance cannot be taken from are ZRT_E_INVALID also
    on a machine with no GPU, where a valid call would end in ZRT_E_NODEVICE; the chunk rule's
    message names sample_chunk as the remedy."""
    _, view, cam = S.get("bubbles")
    ok = z.RenderParams(8, 8, 8, 1, sample_chunk=4)
    with pytest.raises(z.ZrtError) as e:
        z.render_denoised_guided(view, cam, ok, denoise=_ffi.Denoise(iterations=9, sigma_color=1.0), flags=0)
    assert e.value.code == _ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:
        z.render_denoised_guided(view, cam, ok, flags=4)
    assert e.value.code == _ffi.ZRT_E_INVALID and "flag" in str(e.value)
    for spp, chunk in ((10, 4), (4, 4), (32, 0), (40, 0), (24, 16)):
        for tol in (None, 0.5):
            with pytest.raises(z.ZrtError) as e:
                z.render_denoised_guided(view, cam, z.RenderParams(8, 8, spp, 1, sample_chunk=chunk), tolerance=tol)
            assert e.value.code == _ffi.ZRT_E_INVALID and "sample_chunk" in str(e.value), (spp, chunk)


# ---- the restatement of the variance plane ------------------------------------------------

def test_variance_restatement_is_the_sample_variance():
    """k chunk sums of c samples: the plane is the unbiased sample variance of the chunk
    brightnesses over k c^2 - the variance of the preview's r + g + b - to f32 accuracy; a
    constant pixel gives 0 (clamped), a NaN sum gives NaN."""
    rng = np.random.default_rng(11)
    c, k = 4, 8
    sums = (rng.random((k, 5, 6, 3), dtype=F) * F(c)).astype(F)
    sums[:, 0, 0] = F(1.5)
    sums[3, 1, 1, 2] = np.nan
    acc, q = G.accumulate(sums)
    var = G.variance(acc, q, c, k)
    assert var.dtype == np.float32 and var[0, 0] == 0 and np.isnan(var[1, 1]) and np.isnan(var).sum() == 1
    l = sums.astype(np.float64).sum(axis=3)
    want = l.var(axis=0, ddof=1) / (k * c * c)
    ok = ~np.isnan(want)
    ok[0, 0] = False
    assert np.allclose(var[ok], want[ok], rtol=1e-4, atol=0)


# ---- the restatement of the guided filter -------------------------------------------------

def _flat_features(h, w, prim=3):
    f = np.zeros((h, w, 8), F)
    f[..., 2] = 1.0
    f[..., 3] = 2.0
    f[..., 4:7] = 0.5
    f[..., 7] = np.array([prim + 1], np.uint32).view(F)[0]
    return f


def synthetic(h, w, seed):
    """tests/test_gpu_denoise.py's synthetic buffers (a normal edge, a depth step, a checkered
    albedo, a miss corner) plus a seeded positive variance plane."""
    rng = np.random.default_rng(seed)
    frame = rng.random((h, w, 3), dtype=F)
    f = np.zeros((h, w, 8), F)
    x = np.arange(w)[None, :].repeat(h, 0)
    y = np.arange(h)[:, None].repeat(w, 1)
    left = x < max(1, w // 2)
    f[..., 0:3] = np.where(left[..., None], np.array([0.0, 0.0, 1.0], F), np.array([0.6, 0.0, 0.8], F))
    f[..., 0:3] += (rng.random((h, w, 3), dtype=F) - F(0.5)) * F(0.05)
    f[..., 3] = np.where(y < max(1, h // 2), F(2.0), F(5.0)) + rng.random((h, w), dtype=F) * F(0.2)
    f[..., 4:7] = np.where(((x // 5 + y // 7) % 2 == 0)[..., None], F(0.8), F(0.3)) + rng.random((h, w, 3), dtype=F) * F(0.1)
    ids = (1 + (x // 6) + 16 * (y // 6)).astype(np.uint32)
    miss = (x >= w - max(1, w // 4)) & (y >= h - max(1, h // 4)) & (h > 1)
    ids[miss] = 0
    f[..., 7] = ids.view(F)
    f[miss, 0:4] = 0.0
    var = (rng.random((h, w), dtype=F) * F(0.05) + F(0.001)).astype(F)
    return frame, f, var


@pytest.mark.parametrize("value", [1.0, 0.75, 123.5, 59.0 / 8192.0, 4095.0 / 4096.0])
def test_constant_frame_with_zero_variance_stays_constant(value):
    """tests/test_denoise_host.py's exactness argument carries over with the colour term ON: on
    a constant frame every luminance difference is 0, so t_c = 1 - 0 * kl = 1 whatever kl is
    (2^20 for a zero variance) and every weight is h(dx) h(dy) as with all terms off; the
    filtered variance of a zero plane is 0."""
    c = np.full((13, 17, 3), value, F)
    zero = np.zeros((13, 17), F)
    for iters in (1, 3, 5, 8):
        out, ov = G.guided(c, _flat_features(13, 17), zero, iters, 1.0, 0.0, 0.0, 0.0)
        assert out.dtype == np.float32 and (out == c).all() and (ov == 0).all()


@pytest.mark.parametrize("terms", [(0.25, 0.5, 0.25), (0.0, 0.0, 0.0), (0.25, 0.0, 0.0)])
def test_guided_without_its_colour_term_is_the_plain_filter(terms):
    """sigma_color 0, no flag: the variance guides nothing, and the colours are denoise_ref.atrous
    with its colour term off, bit for bit."""
    frame, feat, var = synthetic(24, 40, 7)
    for iters in (1, 3, 5):
        got, gv = G.guided(frame, feat, var, iters, 0.0, *terms)
        want = R.atrous(frame, feat, iters, 0.0, *terms)
        assert (bits(got) == bits(want)).all()
        assert (gv[:, 24:] == var[:, 24:]).all() and (gv[:, :24] != var[:, :24]).any()


def test_demodulation_alone_comes_back_within_four_roundings():
    """Demodulation is not required to round-trip: (x / A) * A need not be x in f32.  With every
    tap but the centre failing (distinct depths against a tiny sigma_depth, one iteration) a
    pixel goes through x / A, * w0, / w0, * A - four roundings - so it comes back within
    4 x 2^-24 relative (to first order), and where the flag changes nothing (a miss, an albedo
    channel at or below a_min) it is bit for bit the unflagged filter's."""
    h = w = 12
    frame, feat, var = synthetic(h, w, 9)
    feat[..., 3] = (1.0 + np.arange(h * w, dtype=F)).reshape(h, w)
    ids = np.ones((h, w), np.uint32)
    ids[3, 4] = 0  # one isolated miss
    feat[..., 7] = ids.view(F)
    feat[2, 2, 4:7] = (0.0, float(G.A_MIN), float(np.nextafter(G.A_MIN, F(1.0))))
    args = (1, 0.0, 0.0, 0.0, 2.0 ** -20)
    plain, pv = G.guided(frame, feat, var, *args, flags=0)
    dem, dv = G.guided(frame, feat, var, *args, flags=G.DEMODULATE)
    rel = np.abs(dem.astype(np.float64) - frame) / frame
    assert rel.max() <= 4.01 * 2.0 ** -24
    assert (np.abs(dv.astype(np.float64) - var) / var).max() <= 6.01 * 2.0 ** -24  # (am * am and w0 * w0 twice more)
    same = np.zeros((h, w, 3), bool)
    same[3, 4] = True
    same[2, 2, 0:2] = True
    assert (bits(dem)[same] == bits(plain)[same]).all()
    assert bits(dv)[3, 4] == bits(pv)[3, 4]


def test_nan_variance_never_reaches_the_colours():
    """A NaN variance pixel: with the colour term on, its own taps and its neighbours' fail (g is
    NaN), so they keep their colours through the centre tap; no colour becomes NaN in any
    iteration; the NaN spreads in the variance plane only."""
    frame, feat, var = synthetic(24, 24, 10)
    feat = _flat_features(24, 24)
    var[11, 9] = np.nan
    out, ov = G.guided(frame, feat, var, 1, 1.0, 0.0, 0.0, 0.0)
    assert not np.isnan(out).any() and np.isnan(ov[11, 9])
    w0 = R.H5[2] * R.H5[2]
    for y, x in ((11, 9), (10, 8), (12, 10), (11, 10)):
        assert (bits(out[y, x]) == bits((frame[y, x] * w0) / w0)).all()
    out5, ov5 = G.guided(frame, feat, var, 5, 1.0, 0.0, 0.0, 0.0)
    assert not np.isnan(out5).any() and np.isnan(ov5).sum() > 1
    # a NaN colour pixel stays where it is, as in the plain filter
    frame[5, 7, 1] = np.nan
    var[11, 9] = 0.01
    out, _ = G.guided(frame, feat, var, 3, 1.0, 0.0, 0.0, 0.0)
    assert np.isnan(out[5, 7, 1]) and np.isnan(out).sum() == 1

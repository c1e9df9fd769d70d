"""Host-side tests of the denoiser (no GPU): the defaults, every refusal, the ctypes
layout, and the numpy restatements of tests/denoise_ref.py that the GPU tests compare
the kernels against."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

import denoise_ref as R
import shading_scenes as S

REPO = z.REPO
F = np.float32


def test_defaults_are_the_probes_winner():
    d = z.denoise_defaults()
    assert d.iterations == 5
    with open(os.path.join(REPO, "profiles", "r10", "denoise", "defaults.json")) as f:
        rec = json.load(f)
    for k in ("sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"):
        v = getattr(d, k)
        assert math.isfinite(v) and v >= 0.0
        assert v == rec["winner"][k], k
        assert v == 0.0 or math.log2(v) == int(math.log2(v))  # the grid is powers of two
    assert list(d.reserved) == [0, 0, 0]


def test_denoise_struct_matches_the_header():
    src = open(os.path.join(REPO, "include", "zrt.h")).read()
    body = re.search(r"typedef struct zrt_denoise \{(.*?)\} zrt_denoise;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|float)\s+(\w+)(\[\d+\])?;", body)
    assert [n for _, n, _ in fields] == [n for n, _ in _ffi.Denoise._fields_]
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    for (t, n, arr), (fn, ft) in zip(fields, _ffi.Denoise._fields_):
        assert ft == (ctype[t] * int(arr[1:-1]) if arr else ctype[t]), n
    assert C.sizeof(_ffi.Denoise) == 32
    assert "#define ZRT_ABI_VERSION 2" in src and z.lib().zrt_abi_version() == 2
    assert "ZRT_DEFAULT_DENOISE_ITERATIONS = 5u" in src


def _denoise_rc(width=8, height=8, frame=0x1000, feat=0x2000, out=0x3000, **fields):
    """zrt_ctx_denoise with no context: what it refuses of its arguments comes first."""
    dn = _ffi.Denoise(iterations=1, sigma_color=1.0, sigma_normal=1.0, sigma_albedo=1.0, sigma_depth=1.0)
    for k, v in fields.items():
        setattr(dn, k, v)
    p = z.RenderParams(width, height, 1, 1).abi()
    rc = z.lib().zrt_ctx_denoise(None, C.byref(p), C.byref(dn), C.c_void_p(frame), C.c_void_p(feat), C.c_void_p(out),
                                 None)
    return rc, z.lib().zrt_last_error().decode()


@pytest.mark.parametrize("field", ["sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"])
@pytest.mark.parametrize("value", [-1.0, -0.0 - 1e-30, float("nan"), float("inf"), float("-inf")])
def test_bad_sigma_is_refused(field, value):
    rc, msg = _denoise_rc(**{field: value})
    assert rc == _ffi.ZRT_E_INVALID and field in msg


def test_other_refusals():
    rc, msg = _denoise_rc(iterations=9)
    assert rc == _ffi.ZRT_E_INVALID and "iterations" in msg
    rc, msg = _denoise_rc(width=8, height=9)
    assert rc == _ffi.ZRT_E_INVALID and "height > width" in msg
    rc, msg = _denoise_rc(out=0x1000)
    assert rc == _ffi.ZRT_E_INVALID and "dev_out must not be dev_frame" in msg
    rc, msg = _denoise_rc(feat=0x2004)
    assert rc == _ffi.ZRT_E_INVALID and "aligned" in msg
    # what is valid gets as far as the missing context
    rc, msg = _denoise_rc(iterations=8, sigma_color=0.0, sigma_depth=0.0)
    assert rc == _ffi.ZRT_E_INVALID and msg == "null argument"
    rc, msg = _denoise_rc(iterations=0)
    assert rc == _ffi.ZRT_E_INVALID and msg == "null argument"


def test_render_denoised_refuses_before_any_device_work():
    """A bad zrt_denoise is ZRT_E_INVALID from the one-shot call too - also on a machine
    with no GPU, where a valid call would end in ZRT_E_NODEVICE."""
    _, view, cam = S.get("bubbles")
    p = z.RenderParams(8, 8, 1, 1)
    for bad in (_ffi.Denoise(iterations=9, sigma_color=1.0), _ffi.Denoise(iterations=1, sigma_normal=float("nan")),
                _ffi.Denoise(iterations=1, sigma_depth=-0.5)):
        with pytest.raises(z.ZrtError) as e:
            z.render_denoised(view, cam, p, denoise=bad)
        assert e.value.code == _ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:
        z.render_denoised(view, cam, z.RenderParams(8, 9, 1, 1))
    assert e.value.code == _ffi.ZRT_E_INVALID


def _flat_features(h, w, prim=3):
    f = np.zeros((h, w, 8), F)
    f[..., 2] = 1.0
    f[..., 3] = 2.0
    f[..., 4:7] = 0.5
    f[..., 7] = np.array([prim + 1], np.uint32).view(F)[0]
    return f


@pytest.mark.parametrize("value", [1.0, 0.75, 123.5, 59.0 / 8192.0, 4095.0 / 4096.0])
def test_constant_frame_stays_constant(value):
    """All terms off: every tap's weight is h(dx) h(dy) and acc / wsum comes back within
    1 ulp of the constant - in the corners (9 taps) as in the middle, after any number of
    iterations.  The constants have at most 12 significant bits: the weights are k / 256
    with k <= 36 = 9 x 4, so every product c w has at most 16 bits and every partial sum of
    up to 25 of them at most 21, all exact in f32, and so is wsum; acc = c wsum exactly and
    the quotient is c.  (No such bound holds for a constant of 24 significant bits: the 24
    additions each round, and a frame of 0.00725 comes back up to 2 ulp off - that is the
    definition's arithmetic, which the GPU tests pin bit for bit.)"""
    c = np.full((13, 17, 3), value, F)
    assert float(F(value)) == value
    for iters in (1, 3, 5, 8):
        out = R.atrous(c, _flat_features(13, 17), iters, 0.0, 0.0, 0.0, 0.0)
        assert out.dtype == np.float32
        ulp = np.spacing(F(value))
        assert np.abs(out.astype(np.float64) - float(F(value))).max() <= float(ulp)
        assert (out == c).all()  # (exact, by the argument above)


def test_normal_edge_separates_the_two_sides():
    """sigma_normal so small that t_n <= 0 across the edge: no tap crosses it, so new
    colours on the right leave the left side's output bit-identical."""
    h = w = 20
    f = _flat_features(h, w)
    f[:, 10:, 0:3] = (0.6, 0.0, 0.8)  # |dN|^2 = 0.36 + 0.04 = 0.4 against (0, 0, 1)
    sigma_n = 0.25  # t_n = 1 - 0.4 / 0.25 < 0
    rng = np.random.default_rng(5)
    a = rng.random((h, w, 3), dtype=F)
    b = a.copy()
    b[:, 10:] = rng.random((h, 10, 3), dtype=F) * F(4.0)
    oa = R.atrous(a, f, 5, 0.0, sigma_n, 0.0, 0.0)
    ob = R.atrous(b, f, 5, 0.0, sigma_n, 0.0, 0.0)
    assert (oa[:, :10].view(np.uint32) == ob[:, :10].view(np.uint32)).all()
    assert (oa[:, 10:] != ob[:, 10:]).any()
    # with the term off the sides mix
    oc = R.atrous(b, f, 5, 0.0, 0.0, 0.0, 0.0)
    assert (oc[:, :10] != oa[:, :10]).any()


def test_nan_stays_where_it_is():
    """A NaN neighbour is skipped by the colour term's comparison; the pixel's own NaN
    survives through the untested centre tap."""
    rng = np.random.default_rng(6)
    a = rng.random((12, 12, 3), dtype=F)
    a[5, 7, 1] = np.nan
    out = R.atrous(a, _flat_features(12, 12), 3, 1.0, 0.0, 0.0, 0.0)
    nan = np.isnan(out)
    assert nan[5, 7, 1] and nan.sum() == 1


@pytest.mark.parametrize("name", ["bubbles", "wraps"])
def test_triangle_uv_restatement(name):
    """denoise_ref.triangle_uv against the oracle: a + u (b - a) + v (c - a) lies within
    1e-4 of the triangle's size of the hit location oracle_triangle_hit reports, over the
    rays the GPU tests use (the 24 x 24 frame's image-textured triangle hits)."""
    s, view, cam = S.get(name)
    feat, tri = R.expected_features(O, view, cam, 24, 24)
    assert len(tri) >= 10
    for a, b, c, o, d, u, v, loc in tri:
        a, b, c = (np.asarray(x, np.float64) for x in (a, b, c))
        size = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b))
        p = a + float(u) * (b - a) + float(v) * (c - a)
        assert np.linalg.norm(p - loc.astype(np.float64)) <= 1e-4 * size
        assert 0.0 <= u and 0.0 <= v and u + v <= 1.0


def test_expected_features_layout():
    """The composed buffer: ids index the scene's list, a miss is (0, 0, background, 0),
    the normal faces the ray, dielectrics are white, columns x >= height stay zero."""
    s, view, cam = S.get("bubbles")
    feat, _ = R.expected_features(O, view, cam, 40, 24)
    assert feat.shape == (24, 40, 8) and feat.dtype == np.float32
    assert (feat[:, 24:] == 0).all()
    ids = np.ascontiguousarray(feat[:, :24, 7]).view(np.uint32)
    assert ids.max() <= s.n_prims and (ids == 0).any() and (ids > 0).any()
    miss = ids == 0
    assert (feat[:, :24, 0:4][miss] == 0).all() and (feat[:, :24, 4:7][miss] > 0).all()
    o, d = R.pixel_rays(cam, 40, 24)
    du = R.unit(d[:, :24])
    n = feat[:, :24, 0:3]
    facing = (du * n).sum(axis=2)
    assert (facing[~miss] <= 0).all()
    glass = [i for i in range(s.n_prims) if s.materials[s.prims[i].material].kind == _ffi.ZRT_MAT_DIELECTRIC]
    is_glass = np.isin(ids, np.array(glass, np.uint32) + 1)
    assert is_glass.any() and (feat[:, :24, 4:7][is_glass] == 1.0).all()

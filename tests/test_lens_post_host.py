"""Host-side tests of the post chain of lens frames (no GPU): the new entry points and their
ctypes signatures, zrt_rect_check, every refusal that needs no device, and the new numpy
references (tests/lens_post_ref.py) pinned to the ones the existing suites already trust."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

import camera_ref as CR
import denoise_guided_ref as G
import denoise_ref as D
import lens_post_ref as L
import radiance_ref as R
import shading_scenes as S
import test_denoise_guided_host as H

F = np.float32
NEW = ["zrt_rect_check", "zrt_ctx_camera_features", "zrt_ctx_camera_moments", "zrt_ctx_camera_variance",
       "zrt_ctx_denoise_rect", "zrt_render_lens_denoised"]
POSE = ((0.3, 1.6, -3.4), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), 38.0, 1.5)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    return ((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all()


# ---- the interface ----------------------------------------------------------------------

def test_new_symbols_are_exported_and_bound():
    src = open(os.path.join(z.REPO, "include", "zrt.h")).read()
    declared = set(re.findall(r"\b(zrt_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    table = {name for name, _, _ in _ffi.SIGNATURES}
    for name in NEW:
        assert name in declared and name in table, name
        assert getattr(z.lib(), name).argtypes is not None
    assert C.sizeof(_ffi.Rect) == 16
    assert re.search(r"typedef struct zrt_rect \{ uint32_t x0, y0, w, h; \} zrt_rect;", src)
    for name in ("camera_features", "camera_moments", "camera_variance", "denoise_rect"):
        assert callable(getattr(z.RenderContext, name))
    assert callable(z.render_lens_denoised)


# ---- zrt_rect_check -----------------------------------------------------------------------

def rect_rc(p, r):
    pa = p.abi() if p is not None else None
    return z.lib().zrt_rect_check(C.byref(pa) if pa is not None else None, C.byref(r) if r is not None else None)


def test_rect_check():
    p = z.RenderParams(24, 16, 8, 12, sample_chunk=4)
    for r in [(0, 0, 24, 16), (3, 2, 13, 9), (23, 15, 1, 1), (0, 0, 1, 1)]:
        assert rect_rc(p, z.rect(*r)) == 0, r
    # a frame taller than wide is a camera query's frame, whatever the render refuses
    assert rect_rc(z.RenderParams(33, 40, 1, 1), z.rect(0, 0, 33, 40)) == 0
    assert rect_rc(z.RenderParams(65535, 65535, 1, 1), z.rect(65534, 65534, 1, 1)) == 0
    bad = [(0, 0, 0, 16), (0, 0, 24, 0), (24, 0, 1, 1), (0, 16, 1, 1), (3, 2, 22, 9), (3, 2, 13, 15),
           (0xFFFFFFFF, 0, 2, 1), (1, 0, 0xFFFFFFFF, 1), (0, 1, 1, 0xFFFFFFFF)]
    for r in bad:
        assert rect_rc(p, z.rect(*r)) == _ffi.ZRT_E_INVALID, r
    assert rect_rc(None, z.rect(0, 0, 1, 1)) == _ffi.ZRT_E_INVALID
    assert rect_rc(p, None) == _ffi.ZRT_E_INVALID
    for kw in ({"width": 0}, {"height": 0}, {"width": 65536}, {"height": 65536}, {"traversal": 3}, {"prng": 2}):
        q = z.RenderParams(**{"width": 24, "height": 16, "samples_per_pixel": 8, "max_depth": 12, **kw})
        assert rect_rc(q, z.rect(0, 0, 1, 1)) == _ffi.ZRT_E_INVALID, kw
    with pytest.raises(z.ZrtError):
        z.rect_check(p, z.rect(3, 2, 22, 9))


# ---- the one-shot's refusals that need no device ------------------------------------------

def test_render_lens_denoised_refuses_before_any_device_work():
    """ZRT_E_INVALID also on a machine with no GPU, where a valid call ends in ZRT_E_NODEVICE."""
    _, view, _ = S.get("wraps")
    lens = z.lens_init(z.ZRT_LENS_FISHEYE, *POSE)
    ok = z.RenderParams(24, 16, 8, 6, sample_chunk=4)

    def refused(word, p=ok, lens=lens, n=8, **kw):
        with pytest.raises(z.ZrtError) as e:
            z.render_lens_denoised(view, p, lens, n, **kw)
        assert e.value.code == _ffi.ZRT_E_INVALID and word in str(e.value), (str(e.value), kw)

    refused("rectangle", rect=(3, 2, 22, 9))
    refused("rectangle", rect=(3, 2, 0, 9))
    refused("n_samples", n=0)
    refused("iterations", denoise=_ffi.Denoise(iterations=9, sigma_color=1.0))
    refused("sigma_normal", denoise=_ffi.Denoise(iterations=1, sigma_normal=float("nan")))
    refused("flag", flags=2)
    refused("flag", guided=False, flags=z.ZRT_DN_DEMODULATE)  # flags without a variance plane
    # guided: what the variance plan refuses - a ragged total, fewer than two chunks
    refused("sample_chunk", n=9)
    refused("sample_chunk", n=4)
    refused("sample_chunk", p=z.RenderParams(24, 16, 8, 6), n=32)  # the default chunk, 32: one chunk
    bad = z.lens_init(z.ZRT_LENS_FISHEYE, *POSE)
    bad.half_fov = 0.0
    refused("half_fov", lens=bad)


# ---- the new references against the old ---------------------------------------------------

TERMS = {"color": (1, 0, 0, 0), "all": (1, 1, 1, 1), "none": (0, 0, 0, 0), "depth": (0, 0, 0, 1)}


@pytest.mark.parametrize("h,w", [(1, 1), (12, 12), (12, 20), (21, 21)])
@pytest.mark.parametrize("terms", list(TERMS))
def test_rect_filters_on_the_square_are_the_old_references(h, w, terms):
    """D = {0, 0, height, height} in atrous_rect / guided_rect is denoise_ref.atrous' and
    denoise_guided_ref.guided's D: the outputs agree bit for bit, the copied columns included."""
    frame, feat, var = H.synthetic(h, w, 77 * h + w)
    sq = (0, 0, h, h)
    for iters in (1, 3, 5):
        s = [v if o else 0.0 for v, o in zip((0.5, 0.25, 0.5, 0.25), TERMS[terms])]
        assert same(L.atrous_rect(frame, feat, sq, iters, *s), D.atrous(frame, feat, iters, *s)), (terms, iters)
        s[0] = 4.0 if TERMS[terms][0] else 0.0
        for flags in (0, G.DEMODULATE):
            got, gv = L.guided_rect(frame, feat, var, sq, iters, *s, flags)
            want, wv = G.guided(frame, feat, var, iters, *s, flags)
            assert same(got, want) and same(gv, wv), (terms, iters, flags)


def test_rect_filters_skip_taps_outside_the_rectangle():
    """A rectangle inside a frame equals the filter of the cropped frame alone: what lies
    outside D is never a tap; and it is copied."""
    frame, feat, var = H.synthetic(30, 34, 5)
    rect = (5, 3, 17, 11)
    x0, y0, w, h = rect
    crop = (slice(y0, y0 + h), slice(x0, x0 + w))
    s = (4.0, 0.25, 0.5, 0.25)
    got, gv = L.guided_rect(frame, feat, var, rect, 4, *s, G.DEMODULATE)
    alone, av = L.guided_rect(frame[crop], feat[crop], var[crop], (0, 0, w, h), 4, *s, G.DEMODULATE)
    assert same(got[crop], alone) and same(gv[crop], av)
    out = np.ones(frame.shape[:2], bool)
    out[crop] = False
    assert same(got[out], frame[out]) and same(gv[out], var[out])
    assert (got[crop] != frame[crop]).any()
    other = frame.copy()
    other[out] += F(1.0)
    again, _ = L.guided_rect(other, feat, var, rect, 4, *s, G.DEMODULATE)
    assert same(again[crop], got[crop])
    plain = L.atrous_rect(frame, feat, rect, 4, 0.5, 0.25, 0.5, 0.25)
    assert same(plain[crop], L.atrous_rect(frame[crop], feat[crop], (0, 0, w, h), 4, 0.5, 0.25, 0.5, 0.25))
    assert same(plain[out], frame[out])
    # taller than wide: the old references refuse it, the new ones do not
    tall = L.atrous_rect(frame[:, :20], feat[:, :20], (0, 0, 20, 30), 3, 0.5, 0.25, 0.5, 0.25)
    assert tall.shape == (30, 20, 3) and (tall != frame[:, :20]).any()


@pytest.mark.parametrize("name", ["wraps", "glass-inside"])
def test_pinhole_lens_features_on_the_square_are_expected_features(name):
    _, view, cam = S.get(name)
    w, h = 24, 16
    p = z.RenderParams(w, h, 1, 1)
    want, _ = D.expected_features(O, view, cam, w, h)
    for kind in (z.ZRT_LENS_PINHOLE, z.ZRT_LENS_THIN):  # the thin lens at its centre is the pinhole
        lens = z.lens_from_camera(kind, cam, aperture=0.5 if kind else 0.0)
        got = L.expected_lens_features(O, view, lens, p, (0, 0, h, h))
        assert same(got, want), kind
    whole = L.expected_lens_features(O, view, z.lens_from_camera(z.ZRT_LENS_PINHOLE, cam), p)
    assert same(whole[:, :h], want[:, :h]) and whole[:, h:, 4:7].any(), "nothing past the square"


def test_moments_restatement():
    """moments() over [0, 8) then [8, 16) equals [0, 16); a ragged ninth sample enters the
    sums and not Q; its sums are radiance_ref.chunk_sums'; Q and the plane are
    denoise_guided_ref's over the same chunk sums."""
    rng = np.random.default_rng(3)
    cols = rng.random((7, 16, 3), dtype=F)
    whole = L.moments(cols, 4)
    assert same(whole[:, :3], R.chunk_sums(cols, 4)[:, :3])
    two = L.moments(cols[:, 8:], 4, L.moments(cols[:, :8], 4))
    assert same(two, whole)
    nine, eight = L.moments(cols[:, :9], 4), L.moments(cols[:, :8], 4)
    assert same(nine[:, 3], eight[:, 3]) and same(nine[:, :3], R.chunk_sums(cols[:, :9], 4)[:, :3])
    assert (nine[:, :3] != eight[:, :3]).any()
    sums = np.stack([cols[:, 4 * j:4 * j + 4].astype(F) for j in range(4)])  # [chunk, n, 4 samples, 3]
    s = np.zeros((4, 1, 7, 3), F)
    for j in range(4):
        for k in range(4):
            s[j, 0] = s[j, 0] + sums[j][:, k]
    acc, q = G.accumulate(s)
    assert same(whole[:, :3], acc[0]) and same(whole[:, 3], q[0])
    assert same(L.variance_of(whole, 4, 16), G.variance(acc[0], q[0], 4, 4))


def test_centre_rays_are_the_query_rays_at_half_jitter():
    """camera_ref.sample_rays' formula at r1 = r2 = 0.5 gives x / width exactly; the rays of
    an orthographic lens leave the plane, those of the others the origin."""
    p = z.RenderParams(24, 16, 1, 1)
    for kind in range(5):
        lens = z.lens_init(kind, *POSE, aperture=0.8, focus_dist=3.5)
        xs, ys, o, d = L.centre_rays(O, lens, p, (3, 2, 13, 9))
        assert len(xs) == 13 * 9 and xs[0] == 3 and ys[0] == 2 and xs[-1] == 15 and ys[-1] == 10
        assert np.isfinite(d).all() and (np.abs(d).sum(1) > 0).all()
        if kind == z.ZRT_LENS_ORTHO:
            # ((o + axis_w) - o rounds twice: axis_w to a few ulps of the origin's magnitude)
            assert len(np.unique(o, axis=0)) == 13 * 9 and np.abs(d - CR.vec(lens.axis_w)).max() < 1e-6
        else:
            assert (o == CR.vec(lens.origin)).all() and len(np.unique(d, axis=0)) == 13 * 9

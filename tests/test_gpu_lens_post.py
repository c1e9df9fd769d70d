"""GPU tests of the post chain of lens frames (zrt.h "denoising lens frames"), bit for bit
against tests/lens_post_ref.py (composed from the oracle and the numpy restatements):

1. lens features: five models, every traversal and the surface list, the frame and a ragged
   rectangle; 2. the moments of a camera query; 3. the variance plane; 4. both filters on a
   rectangle; 5. the query and context conventions; 6. the one-shot, the wrappers and the CLI.
Frames, scenes and poses are tests/test_gpu_camera.py's.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import camera_ref as CR
import denoise_guided_ref as G
import lens_post_ref as L
import radiance_ref as R
import shading_scenes as S
import test_denoise_guided_host as H
import test_gpu_camera as TC
import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

pytestmark = pytest.mark.gpu
F = np.float32
W, H_, CHUNK = TC.W, TC.H, TC.CHUNK
FILL = TC.FILL
SCENES = TC.SCENES
MODELS = ("pinhole",) + TC.MODELS
TRAVERSALS = TC.TRAVERSALS
RECT = (3, 2, 13, 9)  # straddles tiles, ragged on both sides
DEMOD = z.ZRT_DN_DEMODULATE
cparams, lens_of, ctx_of = TC.cparams, TC.lens_of, TC.ctx_of


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        idx = np.argwhere(~same)
        i = tuple(idx[0])
        raise AssertionError(f"{what}: {len(idx)} of {got.size} values differ, first at {i}: got {got[i]!r} "
                             f"want {want[i]!r}")


def rect_mask(h, w, rect):
    m = np.zeros((h, w), bool)
    m[rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]] = True
    return m


def filled(n, width, value=FILL):
    """A device buffer of n entries of `width` floats plus 16 more entries, all `value`."""
    import torch
    return torch.full((n + 16, width), value, dtype=torch.float32, device="cuda")


def fetch(t, n, what):
    a = t.cpu().numpy()
    assert (a[n:] == F(FILL)).all(), what + ": wrote past the frame"
    return a[:n]


# ---- 1. lens features ----------------------------------------------------------------------

def gpu_lens_features(ctx, p, lens, rect=None, stream=0, sync=True):
    """float32[h, w, 8]; the buffer held FILL before the call."""
    import torch
    n = p.width * p.height
    buf = filled(n, 8)
    torch.cuda.synchronize()
    ctx.camera_features(p, lens, z.rect(*(rect or (0, 0, p.width, p.height))), buf.data_ptr(), stream)
    if sync:
        ctx.sync()
    torch.cuda.synchronize()
    return fetch(buf, n, "lens features").reshape(p.height, p.width, 8)


@functools.lru_cache(maxsize=None)
def want_features(name, model, bvh=True, w=W, h=H_):
    return L.expected_lens_features(O, S.get(name)[1], lens_of(name, model), cparams(w=w, h=h), None, bvh)


@pytest.mark.parametrize("bvh", [True, False], ids=["bvh", "list"])
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("model", MODELS)
def test_lens_features_equal_the_oracle(name, model, bvh):
    want = want_features(name, model, bvh)
    hit = want[..., 7].view(np.uint32) != 0
    assert hit.any() and len(np.unique(want[hit][:, 0:4], axis=0)) > hit.sum() // 2, "a flat buffer"
    if name == "wraps" and model in ("equirect", "fisheye"):  # (the other scene's equirect pose stands inside its glass sphere: every ray hits)
        assert (~hit).any(), "no miss in the frame"
    ctx, lens = ctx_of(name, bvh), lens_of(name, model)
    inside = rect_mask(H_, W, RECT)
    for trav in TRAVERSALS:
        p = cparams(trav=trav, bvh=bvh)
        assert_same_bits(gpu_lens_features(ctx, p, lens), want, f"{name} {model} traversal {trav}: the frame")
        got = gpu_lens_features(ctx, p, lens, RECT)
        assert_same_bits(got[inside], want[inside], f"{name} {model} traversal {trav}: the rectangle")
        assert (got[~inside] == F(FILL)).all(), "a pixel outside the rectangle changed"


def test_thin_lens_features_are_taken_at_the_lens_centre():
    """The thin lens' features are those of the pinhole on the same (focal) plane."""
    name = "wraps"
    thin = lens_of(name, "thin")
    pin = z.lens_init(z.ZRT_LENS_PINHOLE, *TC.POSES[name], focus_dist=3.5)
    ctx, p = ctx_of(name), cparams()
    assert_same_bits(gpu_lens_features(ctx, p, thin), gpu_lens_features(ctx, p, pin), "thin against pinhole")


@pytest.mark.parametrize("name", SCENES)
def test_pinhole_lens_features_on_the_square_are_zrt_ctx_features(name):
    import torch
    cam = S.get(name)[2]
    ctx = ctx_of(name)
    sq = (0, 0, H_, H_)
    for trav in TRAVERSALS:
        p = cparams(trav=trav)
        buf = torch.full((H_ * W * 8,), float("nan"), dtype=torch.float32, device="cuda")
        ctx.features(cam, p, buf.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        old = buf.cpu().numpy().reshape(H_, W, 8)
        got = gpu_lens_features(ctx, p, z.lens_from_camera(z.ZRT_LENS_PINHOLE, cam), sq)
        assert_same_bits(got[:, :H_], old[:, :H_], f"{name} traversal {trav}")
        assert (got[:, H_:] == F(FILL)).all() and (old[:, H_:] == 0).all()


# ---- 2. moments ----------------------------------------------------------------------------

def run_cam(ctx, p, lens, n_samples, rect=None, first_sample=0, into=None, accumulate=False, moments=True):
    """One zrt_ctx_camera_moments (or zrt_ctx_camera) call: (sum float32[w h, 4], rgb float32[w h, 3], info)."""
    import torch
    n = p.width * p.height
    s, c = filled(n, 4), filled(n, 3)
    if into is not None:
        s[:n] = torch.from_numpy(np.ascontiguousarray(into[0], F)).cuda()
        c[:n] = torch.from_numpy(np.ascontiguousarray(into[1], F)).cuda()
    torch.cuda.synchronize()
    q = z.camera_query(*(rect or (0, 0, p.width, p.height)), n_samples, first_sample,
                       z.ZRT_CQ_ACCUMULATE if accumulate else 0)
    (ctx.camera_moments if moments else ctx.camera)(p, lens, q, s.data_ptr(), c.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()
    return fetch(s, n, "sum"), fetch(c, n, "rgb"), ctx.camera_info()


def moment_ref(name, model):
    """The reference frame of 16 samples at depth 12 (the pinhole: test_gpu_camera's own 9)."""
    if model == "pinhole":
        return TC.ref_most(name, model, 0, 12)
    return TC.ref_most(name, model, 0, 12, most=16)


def same_info(a, b):
    return all(a[k] == b[k] for k in R.COUNTERS)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("model", ["pinhole", "thin"])
@pytest.mark.parametrize("n_samples", [8, 9])
def test_moments_equal_the_reference_and_the_camera_query(name, model, n_samples):
    fr = moment_ref(name, model).prefix(n_samples)
    want = L.moments(fr.cols, CHUNK)
    assert_same_bits(want[:, :3], fr.sum[:, :3], "the reference's sums")
    assert (want[:, 3] > 0).any()
    if n_samples == 9:  # the ragged ninth sample enters the sums and not Q
        eight = L.moments(fr.cols[:, :8], CHUNK)
        assert_same_bits(want[:, 3], eight[:, 3], "Q of nine samples")
        assert (want[:, :3] != eight[:, :3]).any()
    ctx, lens = ctx_of(name), lens_of(name, model)
    inside = rect_mask(H_, W, RECT).reshape(-1)
    for trav in TRAVERSALS:
        p = cparams(0, 12, trav)
        plain = run_cam(ctx, p, lens, n_samples, moments=False)
        got = run_cam(ctx, p, lens, n_samples)
        assert_same_bits(got[0][fr.R], want, f"{name} {model} traversal {trav}: sums and Q")
        assert_same_bits(got[1][fr.R], fr.rgb, "rgb")
        assert_same_bits(got[0][:, :3], plain[0][:, :3], "sum.rgb against zrt_ctx_camera")
        assert_same_bits(got[1], plain[1], "rgb against zrt_ctx_camera")
        assert same_info(got[2], plain[2]) and same_info(got[2], fr.info)
        assert (plain[0][:, 3] == 0).all(), "zrt_ctx_camera must leave 0 in sum.w"
        part = run_cam(ctx, p, lens, n_samples, RECT)
        assert_same_bits(part[0][inside], got[0][inside], "the rectangle")
        assert (part[0][~inside] == F(FILL)).all() and (part[1][~inside] == F(FILL)).all()


@pytest.mark.parametrize("name", SCENES)
def test_moments_accumulate(name, monkeypatch):
    """[0, 8) then [8, 16) accumulated equals [0, 16), Q included; the same in several rounds
    (ZRT_RADIANCE_PARTIAL_CAP = one chunk of every slot) and in one block (ZRT_RADIANCE_GRID)."""
    fr = moment_ref(name, "thin")
    want = L.moments(fr.cols, CHUNK)
    assert_same_bits(L.moments(fr.cols[:, 8:], CHUNK, L.moments(fr.cols[:, :8], CHUNK)), want, "the reference, split")
    ctx, lens, p = ctx_of(name), lens_of(name, "thin"), cparams(0, 12)

    def both(what):
        whole = run_cam(ctx, p, lens, 16)
        assert_same_bits(whole[0][fr.R], want, what + ": one call")
        assert_same_bits(whole[1][fr.R], fr.rgb, what + ": rgb")
        first = run_cam(ctx, p, lens, 8)
        assert_same_bits(first[0][fr.R], L.moments(fr.cols[:, :8], CHUNK), what + ": [0, 8)")
        second = run_cam(ctx, p, lens, 8, first_sample=8, into=first[:2], accumulate=True)
        assert_same_bits(second[0], whole[0], what + ": [0, 8) + [8, 16)")
        assert_same_bits(second[1], whole[1], what + ": rgb of the two")
        return whole

    both("plain")
    if name == "wraps":
        slots = 3 * 2 * 64
        cap = slots * 16
        assert z.debug_camera_plan(p, z.camera_query(0, 0, W, H_, 16), 256, cap)["radiance"]["rounds"] == 4
        monkeypatch.setenv("ZRT_RADIANCE_PARTIAL_CAP", str(cap))
        both("four rounds")
        monkeypatch.setenv("ZRT_RADIANCE_PARTIAL_CAP", str(3 * cap))  # 3 chunks, then 1
        both("two rounds")
        nine = run_cam(ctx, p, lens, 9)  # rounds of 3 chunks: the ragged chunk stands alone in the last
        assert_same_bits(nine[0][fr.R], L.moments(fr.cols[:, :9], CHUNK), "nine samples in rounds")
        monkeypatch.delenv("ZRT_RADIANCE_PARTIAL_CAP")
        monkeypatch.setenv("ZRT_RADIANCE_GRID", "1")
        both("one block")
        assert ctx.debug_radiance()["grid"] == 1


# ---- 3. the variance plane -----------------------------------------------------------------

def run_var(ctx, p, rect, n_total, sums, offset_sum=0, offset_var=0, null=None):
    import torch
    n = p.width * p.height
    d_s = torch.from_numpy(np.ascontiguousarray(sums, F)).cuda()
    d_v = filled(n, 1)
    torch.cuda.synchronize()
    ctx.camera_variance(p, z.rect(*rect), n_total, 0 if null == "sum" else d_s.data_ptr() + offset_sum,
                        0 if null == "var" else d_v.data_ptr() + offset_var)
    torch.cuda.synchronize()
    return fetch(d_v, n, "variance")[:, 0]


@pytest.mark.parametrize("name", SCENES)
def test_variance_plane(name):
    fr = moment_ref(name, "thin")
    ctx, lens, p = ctx_of(name), lens_of(name, "thin"), cparams(0, 12)
    inside = rect_mask(H_, W, RECT).reshape(-1)
    for n_total in (8, 16):
        sums = run_cam(ctx, p, lens, n_total)[0]
        want = L.variance_of(L.moments(fr.cols[:, :n_total], CHUNK), CHUNK, n_total)
        assert (want > 0).sum() > W * H_ // 2
        assert_same_bits(run_var(ctx, p, (0, 0, W, H_), n_total, sums)[fr.R], want, f"{n_total} samples")
        got = run_var(ctx, p, RECT, n_total, sums)
        assert (fr.R == np.arange(W * H_)).all()
        assert_same_bits(got[inside], want[inside], "the rectangle")
        assert (got[~inside] == F(FILL)).all()
    # NaN in gives NaN out; a constant pixel clamps at 0
    sums = np.array(sums)
    sums[5] = (np.nan, 1.0, 1.0, 4.0)
    sums[6] = (1.0, 1.0, np.nan, 4.0)
    sums[7] = (1.0, 1.0, 1.0, np.nan)
    sums[8] = (4.0, 4.0, 4.0, 36.0)  # four chunk sums of brightness 3: Q = 36, v = 36 / 4 - 9 = 0
    sums[9] = (4.0, 4.0, 4.0, 35.0)  # v < 0: clamped
    got = run_var(ctx, p, (0, 0, W, H_), 16, sums)
    assert_same_bits(got, G.variance(sums[:, :3], sums[:, 3], CHUNK, 4), "NaN and clamped pixels")
    assert np.isnan(got[5:8]).all() and np.isnan(got).sum() == 3 and got[8] == 0 and got[9] == 0
    for bad in (9, 4, 0, 18):  # ragged totals, a single chunk
        with pytest.raises(z.ZrtError) as e:
            run_var(ctx, p, RECT, bad, sums)
        assert e.value.code == _ffi.ZRT_E_INVALID, bad


# ---- 4. the filters on a rectangle -----------------------------------------------------------

class Filter:
    def __init__(self):
        self.ctx = z.RenderContext(S.get("bubbles")[1], z.RenderParams(8, 8, 1, 1))

    def run(self, frame, feat, var, dn, flags, rect, want_var=True, **bad):
        """zrt_ctx_denoise_rect: (frame, variance or the sentinel plane); var None: the plain filter."""
        import torch
        h, w, _ = frame.shape
        n = h * w
        p = z.RenderParams(w, h, 1, 1)
        d_in = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
        d_ft = torch.zeros(n * 8 + 4, dtype=torch.float32, device="cuda")
        d_ft[:n * 8] = torch.from_numpy(np.ascontiguousarray(feat)).cuda().reshape(-1)
        d_var = torch.from_numpy(np.ascontiguousarray(var)).cuda() if var is not None else None
        d_out, d_ov = filled(n, 3), filled(n, 1)
        torch.cuda.synchronize()
        self.ctx.denoise_rect(p, dn, flags, z.rect(*rect), 0 if bad.get("null_frame") else d_in.data_ptr(),
                              d_ft.data_ptr() + (4 if bad.get("misalign") else 0),
                              d_var.data_ptr() if d_var is not None else 0,
                              d_in.data_ptr() if bad.get("inplace") else d_out.data_ptr(),
                              d_ov.data_ptr() if want_var else 0)
        assert self.ctx.denoise_ms() >= 0.0
        torch.cuda.synchronize()
        return fetch(d_out, n, "out").reshape(h, w, 3), fetch(d_ov, n, "out variance").reshape(h, w)


@pytest.fixture(scope="module")
def filt():
    f = Filter()
    yield f
    f.ctx.close()


# by `guided`: tests/test_gpu_denoise.py's and tests/test_gpu_denoise_guided.py's sigmas
SIGMAS = {False: (0.5, 0.25, 0.5, 0.25), True: (4.0, 0.25, 0.5, 0.25)}
TERMS = {"color": (1, 0, 0, 0), "normal": (0, 1, 0, 0), "albedo": (0, 0, 1, 0), "depth": (0, 0, 0, 1),
         "all": (1, 1, 1, 1), "none": (0, 0, 0, 0)}
# (w, h, rect): one pixel; wider than tall; taller than wide, which the old filters refuse; a rectangle wider
# than one 32-pixel block, shorter than two 8-row blocks, aligned with neither, inside a frame whose pixels
# around it are valid and distinct: far taps of steps 8 and 16 land inside and outside
RECT_CASES = [(1, 1, (0, 0, 1, 1)), (40, 33, (0, 0, 40, 33)), (33, 40, (0, 0, 33, 40)), (70, 70, (5, 3, 37, 11))]


def make_dn(iters, on, guided):
    s = [v if o else 0.0 for v, o in zip(SIGMAS[guided], on)]
    return _ffi.Denoise(iterations=iters, sigma_color=s[0], sigma_normal=s[1], sigma_albedo=s[2], sigma_depth=s[3])


def check_rect(filt, frame, feat, var, dn, flags, rect, what):
    """One call against the restatement, the copied pixels included: (frame, variance)."""
    if var is None:
        got, sentinel = filt.run(frame, feat, None, dn, 0, rect, want_var=False)
        assert_same_bits(got, L.atrous_rect_dn(frame, feat, rect, dn), what)
        assert (sentinel == F(FILL)).all()
        return got, None
    got, gv = filt.run(frame, feat, var, dn, flags, rect)
    want, wv = L.guided_rect_dn(frame, feat, var, rect, dn, flags)
    assert_same_bits(got, want, what)
    assert_same_bits(gv, wv, what + " (variance)")
    return got, gv


@pytest.mark.parametrize("w,h,rect", RECT_CASES, ids=["1x1", "40x33", "33x40", "70x70-rect"])
@pytest.mark.parametrize("terms", list(TERMS))
def test_rect_filters_equal_the_restatement(filt, w, h, rect, terms):
    """Iterations 1 and 3 (the LDS steps 1 and 2, the first step read from memory), 5 and 8."""
    frame, feat, var = H.synthetic(h, w, 1000 * h + w)
    inside = rect_mask(h, w, rect)
    for iters in (1, 3, 5, 8):
        for mode, v, flags in (("plain", None, 0), ("guided", var, 0), ("demodulated", var, DEMOD)):
            dn = make_dn(iters, TERMS[terms], v is not None)
            got, gv = check_rect(filt, frame, feat, v, dn, flags, rect, f"{w}x{h} {rect} {terms} {mode} iterations {iters}")
            assert_same_bits(got[~inside], frame[~inside], "outside pixels are copied")
            if gv is not None:
                assert_same_bits(gv[~inside], var[~inside], "outside variances are copied")
            if h > 1 and iters == 1 and (terms != "none" or v is not None):
                assert (got[inside] != frame[inside]).any()


def test_rect_filters_ignore_what_lies_outside(filt):
    """Other valid values around the rectangle: the rectangle's output does not change."""
    frame, feat, var = H.synthetic(70, 70, 9)
    rect = RECT_CASES[3][2]
    inside = rect_mask(70, 70, rect)
    f2, ft2, v2 = H.synthetic(70, 70, 10)
    for a, b in ((f2, frame), (ft2, feat), (v2, var)):
        a[inside] = b[inside]
    for v, vv, flags in ((None, None, 0), (var, v2, DEMOD)):
        dn = make_dn(5, TERMS["all"], v is not None)
        one, _ = check_rect(filt, frame, feat, v, dn, flags, rect, "frame one")
        two, _ = check_rect(filt, f2, ft2, vv, dn, flags, rect, "frame two")
        assert_same_bits(one[inside], two[inside], "a tap leaked")
        assert (one[~inside] != two[~inside]).any()


def test_rect_filters_nan_pixels(filt):
    frame, feat, var = H.synthetic(70, 70, 4)
    rect = RECT_CASES[3][2]
    f1 = frame.copy()
    f1[7, 20, 2] = np.nan   # inside
    f1[20, 20, 1] = np.nan  # outside: copied, never a tap
    got, _ = check_rect(filt, f1, feat, None, make_dn(5, TERMS["all"], False), 0, rect, "plain, NaN colour")
    assert np.isnan(got[7, 20, 2]) and np.isnan(got[20, 20, 1]) and np.isnan(got).sum() == 2
    got, _ = check_rect(filt, f1, feat, var, make_dn(5, TERMS["all"], True), DEMOD, rect, "guided, NaN colour")
    assert np.isnan(got[7, 20, 2]) and np.isnan(got).sum() == 2
    v1 = var.copy()
    v1[7, 20] = np.nan
    v1[2, 20] = np.nan  # just outside the rectangle's bottom row: the 3 x 3 smoothing must not read it
    got, gv = check_rect(filt, frame, feat, v1, make_dn(5, TERMS["all"], True), 0, rect, "guided, NaN variance")
    assert not np.isnan(got).any() and np.isnan(gv[7, 20]) and np.isnan(gv[2, 20])
    check_rect(filt, f1, feat, var, make_dn(3, TERMS["normal"], True), 0, rect, "guided, NaN colour, no colour term")


def test_rect_filters_on_the_square_are_the_old_filters(filt):
    import torch
    h, w = 24, 40
    frame, feat, var = H.synthetic(h, w, 12)
    p = z.RenderParams(w, h, 1, 1)
    sq = (0, 0, h, h)
    d_in, d_ft, d_var = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (frame, feat, var))
    for iters in (1, 3, 5):
        dn = make_dn(iters, TERMS["all"], False)
        d_out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
        filt.ctx.denoise(p, dn, d_in.data_ptr(), d_ft.data_ptr(), d_out.data_ptr())
        filt.ctx.denoise_ms()
        torch.cuda.synchronize()
        got, _ = filt.run(frame, feat, None, dn, 0, sq, want_var=False)
        assert_same_bits(got, d_out.cpu().numpy(), f"zrt_ctx_denoise, iterations {iters}")
        for flags in (0, DEMOD):
            dn = make_dn(iters, TERMS["all"], True)
            d_ov = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
            filt.ctx.denoise_guided(p, dn, flags, d_in.data_ptr(), d_ft.data_ptr(), d_var.data_ptr(), d_out.data_ptr(),
                                    d_ov.data_ptr())
            filt.ctx.denoise_ms()
            torch.cuda.synchronize()
            got, gv = filt.run(frame, feat, var, dn, flags, sq)
            assert_same_bits(got, d_out.cpu().numpy(), f"zrt_ctx_denoise_guided, iterations {iters}, flags {flags}")
            assert_same_bits(gv, d_ov.cpu().numpy(), "its variance")


# ---- 5. conventions ------------------------------------------------------------------------

@pytest.mark.parametrize("trav", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY], ids=["fast", "binary"])
def test_lens_features_stack_overflow_is_reported(scenes, trav, monkeypatch):
    """As test_gpu_camera.test_stack_overflow_is_reported: NaN in the rectangle only,
    ZRT_E_UNSUPPORTED once, then a correct answer."""
    import torch
    s = scenes(2)
    p = cparams(0, 6, trav, w=16, h=16, spp=2)
    lens = CR.lens_of_camera(s.camera)
    rect = (3, 5, 13, 9)
    inside = rect_mask(16, 16, rect)
    ctx = z.RenderContext(s, p)
    try:
        monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
        got = gpu_lens_features(ctx, p, lens, rect, sync=False)
        with pytest.raises(z.ZrtError) as e:
            ctx.sync()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and "overflow" in str(e.value)
        assert np.isnan(got[inside]).all() and (got[~inside] == F(FILL)).all()
        ctx.sync()  # reported once
        monkeypatch.delenv("ZRT_DEBUG_STACK_CAP")
        buf = torch.zeros(16 * 16 * 8, dtype=torch.float32, device="cuda")
        ctx.features(s.camera, p, buf.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        after = gpu_lens_features(ctx, p, lens, rect)
        assert_same_bits(after[inside], buf.cpu().numpy().reshape(16, 16, 8)[inside], "after the error")
        assert (after[~inside] == F(FILL)).all()
    finally:
        ctx.close()


def test_calls_leave_a_live_run_alone():
    import torch
    name = "wraps"
    view, cam = S.get(name)[1], S.get(name)[2]
    p = z.RenderParams(32, 32, 8, 6, sample_chunk=2)
    pq, lens = cparams(0, 12), lens_of(name, "fisheye")
    fr = TC.ref_most(name, "fisheye", 0, 12, most=5)
    want_f = want_features(name, "fisheye")

    def run_pass(with_calls):
        ctx = z.RenderContext(view, p)
        try:
            tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
            frame = torch.zeros(32 * 32 * 3, dtype=torch.float32, device="cuda")
            ctx.accum_begin(cam, p)
            ctx.accum_pass(4, tiles.data_ptr())
            if with_calls:
                assert_same_bits(gpu_lens_features(ctx, pq, lens), want_f, "features between two passes")
                assert_same_bits(run_cam(ctx, pq, lens, 5)[1][fr.R], fr.rgb, "moments between two passes")
            ctx.accum_pass(4, tiles.data_ptr())
            ctx.assemble(p, tiles.data_ptr(), frame.data_ptr())
            ctx.sync()
            torch.cuda.synchronize()
            out = frame.cpu().numpy().reshape(32, 32, 3).copy(), ctx.stats(), ctx.accum_info()
            if with_calls:
                assert_same_bits(gpu_lens_features(ctx, pq, lens, RECT)[rect_mask(H_, W, RECT)],
                                 want_f[rect_mask(H_, W, RECT)], "features after the run")
                assert all(ctx.stats()[k] == out[1][k] for k in TC.STAT_KEYS), "a call changed zrt_ctx_stats"
            return out
        finally:
            ctx.close()

    plain, st0, info0 = run_pass(False)
    mixed, st1, info1 = run_pass(True)
    assert np.array_equal(plain.view(np.uint32), mixed.view(np.uint32))
    for k in TC.STAT_KEYS:
        assert st0[k] == st1[k], k
    strip = lambda d: {k: v for k, v in d.items() if not k.endswith("_ms")}
    assert strip(info0) == strip(info1)


def test_refusals_on_a_context(filt):
    import torch
    ctx, p, lens = ctx_of("wraps"), cparams(), lens_of("wraps", "thin")
    n = W * H_
    s = torch.zeros((n + 1, 4), dtype=torch.float32, device="cuda")
    f = torch.zeros((n + 1) * 8, dtype=torch.float32, device="cuda")
    v = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    whole = z.rect(0, 0, W, H_)

    def refused(fn, *a):
        with pytest.raises(z.ZrtError) as e:
            fn(*a)
        assert e.value.code == _ffi.ZRT_E_INVALID, a

    refused(ctx.camera_features, p, lens, whole, 0)
    refused(ctx.camera_features, p, lens, whole, f.data_ptr() + 4)
    refused(ctx.camera_features, p, lens, z.rect(0, 0, W + 1, H_), f.data_ptr())
    refused(ctx.camera_features, p, lens, z.rect(3, 2, 0, 9), f.data_ptr())
    refused(ctx.camera_features, cparams(bvh=False), lens, whole, f.data_ptr())  # params that do not fit the context
    bad = z.lens_init(z.ZRT_LENS_THIN, *TC.POSES["wraps"])
    bad.kind = 5
    refused(ctx.camera_features, p, bad, whole, f.data_ptr())
    q = z.camera_query(0, 0, W, H_, 8)
    refused(ctx.camera_moments, p, lens, q, 0)
    refused(ctx.camera_moments, p, lens, q, s.data_ptr() + 4)
    refused(ctx.camera_moments, p, lens, z.camera_query(0, 0, W, H_, 8, flags=2), s.data_ptr())
    refused(ctx.camera_moments, p, lens, z.camera_query(0, 0, W, H_, 8, flags=3), s.data_ptr())
    refused(ctx.camera_moments, p, lens, z.camera_query(0, 0, W, H_, 8, 2, z.ZRT_CQ_ACCUMULATE), s.data_ptr())
    refused(ctx.camera_variance, p, whole, 8, 0, v.data_ptr())
    refused(ctx.camera_variance, p, whole, 8, s.data_ptr(), 0)
    refused(ctx.camera_variance, p, whole, 8, s.data_ptr() + 4, v.data_ptr())
    refused(ctx.camera_variance, p, whole, 8, s.data_ptr(), v.data_ptr() + 2)
    refused(ctx.camera_variance, p, z.rect(0, 0, W, H_ + 1), 8, s.data_ptr(), v.data_ptr())
    torch.cuda.synchronize()
    assert not s.cpu().numpy().any() and not f.cpu().numpy().any() and not v.cpu().numpy().any(), "a refused call wrote"
    # the filter: its pointers, its flags and its rectangle
    frame, feat, var = H.synthetic(24, 24, 6)
    sq = (0, 0, 24, 24)
    dn = make_dn(1, TERMS["all"], True)
    for kw in ({"inplace": True}, {"misalign": True}, {"null_frame": True}):
        refused(lambda: filt.run(frame, feat, var, dn, 0, sq, **kw))
    refused(lambda: filt.run(frame, feat, var, dn, 2, sq))                    # an unknown flag
    refused(lambda: filt.run(frame, feat, None, dn, DEMOD, sq, want_var=False))  # flags without a variance plane
    refused(lambda: filt.run(frame, feat, None, dn, 0, sq, want_var=True))       # an output variance without one
    refused(lambda: filt.run(frame, feat, var, dn, 0, (0, 0, 25, 24)))
    refused(lambda: filt.run(frame, feat, var, dn, 0, (0, 0, 0, 24)))
    refused(lambda: filt.run(frame, feat, var, _ffi.Denoise(iterations=9, sigma_color=1.0), 0, sq))
    refused(lambda: filt.run(frame, feat, var, _ffi.Denoise(iterations=1, sigma_color=float("nan")), 0, sq))
    check_rect(filt, frame, feat, var, dn, 0, sq, "the filter after the refusals")


# ---- 6. end to end -------------------------------------------------------------------------

EW, EH, ESPP = 32, 24, 8


def e2e_reference(view, fr, lens, p, rect, dn_plain, dn_guided, flags):
    """(noisy, features, variance, plain, guided) frames of the reference, zero outside rect."""
    h, w = p.height, p.width
    inside = rect_mask(h, w, rect).reshape(-1)
    keep = inside[fr.R]
    noisy = np.zeros((h * w, 3), F)
    noisy[fr.R[keep]] = fr.rgb[keep]
    noisy = noisy.reshape(h, w, 3)
    feat = L.expected_lens_features(O, view, lens, p, rect)
    var = np.zeros(h * w, F)
    var[fr.R[keep]] = L.variance_of(L.moments(fr.cols, p.sample_chunk), p.sample_chunk, fr.cols.shape[1])[keep]
    var = var.reshape(h, w)
    plain = L.atrous_rect_dn(noisy, feat, rect, dn_plain)
    guided, _ = L.guided_rect_dn(noisy, feat, var, rect, dn_guided, flags)
    return noisy, feat, var, plain, guided


def test_one_shot_and_wrappers():
    import torch
    name, model = "wraps", "fisheye"
    view, lens = S.get(name)[1], lens_of(name, model)
    fr = TC.ref_most(name, model, 0, 12, w=EW, h=EH, most=ESPP)
    p = cparams(0, 12, w=EW, h=EH)
    dn_p = z.denoise_defaults()
    dn_g, flags_g = z.denoise_guided_defaults()
    for rect in ((0, 0, EW, EH), (3, 2, 13, 9)):
        noisy, feat, var, plain, guided = e2e_reference(view, fr, lens, p, rect, dn_p, dn_g, flags_g)
        inside = rect_mask(EH, EW, rect)
        assert (guided[inside] != noisy[inside]).any() and (plain[inside] != noisy[inside]).any()
        lens_rgb, _ = z.render_lens(view, p, lens, ESPP, rect=rect)
        got, out = z.render_lens_denoised(view, p, lens, ESPP, rect=rect)
        assert_same_bits(out["noisy"], noisy, f"guided {rect}: noisy")
        assert_same_bits(out["noisy"], lens_rgb, "noisy against render_lens")
        assert_same_bits(out["features"], feat, "features")
        assert_same_bits(out["variance"], var, "variance")
        assert_same_bits(got, guided, "the guided frame")
        assert out["info"]["samples"] == rect[2] * rect[3] * ESPP and out["denoise_ms"] >= 0
        got, out = z.render_lens_denoised(view, p, lens, ESPP, rect=rect, guided=False)
        assert_same_bits(out["noisy"], lens_rgb, "plain: noisy against render_lens")
        assert_same_bits(out["features"], feat, "plain: features")
        assert_same_bits(got, plain, "the plain frame")
        assert out["variance"] is None
    # flags 0 through the one-shot, and the same chain through the context's wrappers
    rect = (0, 0, EW, EH)
    noisy, feat, var, _, guided0 = e2e_reference(view, fr, lens, p, rect, dn_p, dn_g, 0)
    got, _ = z.render_lens_denoised(view, p, lens, ESPP, flags=0)
    assert_same_bits(got, guided0, "the guided frame, flags 0")
    ctx = z.RenderContext(view, p)
    try:
        n = EW * EH
        s, c, f, v, o, ov = (torch.zeros(n * k, dtype=torch.float32, device="cuda") for k in (4, 3, 8, 1, 3, 1))
        r = z.rect(*rect)
        ctx.camera_moments(p, lens, z.camera_query(*rect, ESPP), s.data_ptr(), c.data_ptr())
        ctx.sync()
        ctx.camera_features(p, lens, r, f.data_ptr())
        ctx.camera_variance(p, r, ESPP, s.data_ptr(), v.data_ptr())
        ctx.denoise_rect(p, dn_g, 0, r, c.data_ptr(), f.data_ptr(), v.data_ptr(), o.data_ptr(), ov.data_ptr())
        ctx.sync()
        assert ctx.denoise_ms() >= 0
        torch.cuda.synchronize()
        assert_same_bits(o.cpu().numpy().reshape(EH, EW, 3), guided0, "the wrappers' frame")
        assert_same_bits(ov.cpu().numpy().reshape(EH, EW), L.guided_rect_dn(noisy, feat, var, rect, dn_g, 0)[1],
                         "the wrappers' variance")
    finally:
        ctx.close()


CLI_DROP = TC.CLI_DROP + ("ZRT_LENS_DENOISE",)


def test_cli_lens_denoise(scenes, tmp_path):
    """zrt-raytrace 32 24 8 5 1 out.png with ZRT_LENS=fisheye, ZRT_LENS_OUT and ZRT_LENS_DENOISE on
    scene 1: the PNG of the reference's filtered frame, per mode; the frame beside it is unchanged."""
    s = scenes(1)
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    env = {k: v for k, v in os.environ.items() if k not in CLI_DROP}
    env.update(ZRT_SAMPLE_CHUNK="4", ZRT_LENS="fisheye", ZRT_FISHEYE_FOV="150", ZRT_LENS_OUT=str(tmp_path / "lens.png"))
    args = [exe, str(EW), str(EH), str(ESPP), "5", "1"]
    p = z.RenderParams(EW, EH, ESPP, 5, sample_chunk=4)
    lens = TC.lens_from_restatement(z.ZRT_LENS_FISHEYE, s.camera, 0.0, 0.0, 150.0)
    fr = CR.Frame(O, s.view, p, lens, ESPP)
    dn_g, _ = z.denoise_guided_defaults()
    rect = (0, 0, EW, EH)
    r = subprocess.run(args + [str(tmp_path / "plain.png")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    unfiltered = (tmp_path / "lens.png").read_bytes()
    seen = {unfiltered}
    for mode, flags in (("plain", None), ("guided", 0), ("demod", DEMOD)):
        noisy, feat, var, plain, guided = e2e_reference(s.view, fr, lens, p, rect, z.denoise_defaults(), dn_g, flags or 0)
        r = subprocess.run(args + [str(tmp_path / "out.png")], env={**env, "ZRT_LENS_DENOISE": mode}, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert f"  Lens frame filter:     {mode}" in r.stderr and f"{fr.info['rays']} rays" in r.stderr
        assert (tmp_path / "out.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
        z.write_png(str(tmp_path / "want.png"), np.ascontiguousarray(plain if flags is None else guided))
        png = (tmp_path / "lens.png").read_bytes()
        assert png == (tmp_path / "want.png").read_bytes(), mode
        seen.add(png)
    assert len(seen) == 4, "two modes wrote the same picture"
    # refused before anything is rendered: without the lens, an unknown mode, a ragged or single-chunk total
    base = {k: v for k, v in env.items() if k not in ("ZRT_LENS", "ZRT_LENS_OUT", "ZRT_FISHEYE_FOV")}
    for bad, spp in (({**base, "ZRT_LENS_DENOISE": "guided"}, "8"), ({**env, "ZRT_LENS_DENOISE": "median"}, "8"),
                     ({**env, "ZRT_LENS_DENOISE": "guided"}, "9"), ({**env, "ZRT_LENS_DENOISE": "demod"}, "4")):
        r = subprocess.run([exe, str(EW), str(EH), spp, "5", "1", str(tmp_path / "refused.png")], env=bad,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "lens frame" in r.stderr, bad
        assert not (tmp_path / "refused.png").exists()
    r = subprocess.run([exe, str(EW), str(EH), "9", "5", "1", str(tmp_path / "nine.png")],
                       env={**env, "ZRT_LENS_DENOISE": "plain"}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr  # the plain filter takes any sample count

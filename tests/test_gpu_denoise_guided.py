"""GPU tests of the variance-guided filter: zrt_ctx_denoise_guided bit for bit against its
numpy restatement (tests/denoise_guided_ref.guided) on synthetic buffers, the one-shot
entry point and the command-line client end to end against the oracle-derived variance
plane, and the quality condition the guided defaults were chosen under
(tools/denoise_guided_probe.py)."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O  # noqa: F401  (the oracle behind the expected planes)

import denoise_guided_ref as G
import denoise_ref as R
import shading_scenes as S
import test_denoise_guided_host as H
import test_gpu_adaptive as A
import test_gpu_denoise as D
import test_gpu_variance as V

pytestmark = pytest.mark.gpu
F = np.float32
DEMOD = z.ZRT_DN_DEMODULATE

assert_same_bits = D.assert_same_bits


class Filter:
    """One context and its device buffers, for many small calls."""

    def __init__(self):
        _, view, _ = S.get("bubbles")
        self.ctx = z.RenderContext(view, z.RenderParams(8, 8, 1, 1))

    def run(self, frame, feat, var, dn, flags=0, want_var=True, inplace=False, null_var=False, misalign=False):
        """(filtered frame, filtered variance or the untouched sentinel plane)."""
        import torch
        h, w, _ = frame.shape
        p = z.RenderParams(w, h, 1, 1)
        d_in = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
        d_ft = torch.zeros(h * w * 8 + 4, dtype=torch.float32, device="cuda")
        d_ft[:h * w * 8] = torch.from_numpy(np.ascontiguousarray(feat)).cuda().reshape(-1)
        d_var = torch.from_numpy(np.ascontiguousarray(var)).cuda()
        d_out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
        d_ov = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
        self.ctx.denoise_guided(p, dn, flags, d_in.data_ptr(), d_ft.data_ptr() + (4 if misalign else 0),
                                0 if null_var else d_var.data_ptr(), d_in.data_ptr() if inplace else d_out.data_ptr(),
                                d_ov.data_ptr() if want_var else 0)
        ms = self.ctx.denoise_ms()
        torch.cuda.synchronize()
        assert ms >= 0.0
        return d_out.cpu().numpy(), d_ov.cpu().numpy()


@pytest.fixture(scope="module")
def filt():
    f = Filter()
    yield f
    f.ctx.close()


# colour (in standard deviations of the brightness: the planes of H.synthetic hold 0.001 .. 0.051,
# brightness differences reach 3), normal, albedo, relative depth - as tests/test_gpu_denoise.py's
SIGMAS = (4.0, 0.25, 0.5, 0.25)
TERMS = D.TERMS


def make_dn(iters, on):
    s = [v if o else 0.0 for v, o in zip(SIGMAS, on)]
    return _ffi.Denoise(iterations=iters, sigma_color=s[0], sigma_normal=s[1], sigma_albedo=s[2], sigma_depth=s[3])


def check(filt, frame, feat, var, dn, flags, what):
    got, gv = filt.run(frame, feat, var, dn, flags)
    want, wv = G.guided_dn(frame, feat, var, dn, flags)
    assert_same_bits(got, want, what)
    assert_same_bits(gv, wv, what + " (variance)")
    return got, gv


@pytest.mark.parametrize("flags", [0, DEMOD], ids=["plain", "demodulated"])
@pytest.mark.parametrize("h,w", [(1, 1), (8, 8), (33, 40), (70, 70)], ids=["1x1", "8x8", "40x33", "70x70"])
@pytest.mark.parametrize("terms", list(TERMS))
def test_guided_filter_equals_the_restatement(filt, h, w, terms, flags):
    """Iterations 1 and 3 (the LDS steps 1 and 2, the first step read from memory), 5 and 8 (step
    128); 33 rows and 70 x 70 cross block and halo boundaries, 40 x 33 has columns outside D."""
    frame, feat, var = H.synthetic(h, w, 1000 * h + w)
    for iters in (1, 3, 5, 8):
        dn = make_dn(iters, TERMS[terms])
        got, gv = check(filt, frame, feat, var, dn, flags, f"{w}x{h} {terms} iterations {iters} flags {flags}")
        if h > 1 and iters == 1:
            assert (got[:, :h] != frame[:, :h]).any() and (gv[:, :h] != var[:, :h]).any()
        if w > h:
            assert (got[:, h:] == frame[:, h:]).all() and (gv[:, h:] == var[:, h:]).all()


def test_guided_colour_term_does_something(filt):
    """The colour term on against off, and a larger variance against a smaller one: different frames."""
    frame, feat, var = H.synthetic(33, 40, 21)
    on, _ = check(filt, frame, feat, var, make_dn(3, TERMS["color"]), 0, "colour on")
    off, _ = check(filt, frame, feat, var, make_dn(3, TERMS["none"]), 0, "colour off")
    big, _ = check(filt, frame, feat, (var * F(64.0)).astype(F), make_dn(3, TERMS["color"]), 0, "64 x variance")
    assert (on != off).any() and (on != big).any()


def test_guided_default_iterations_and_null_out_variance(filt):
    frame, feat, var = H.synthetic(24, 24, 3)
    dn0, dn5 = make_dn(0, TERMS["all"]), make_dn(5, TERMS["all"])
    want, _ = G.guided_dn(frame, feat, var, dn5, DEMOD)
    got, sentinel = filt.run(frame, feat, var, dn0, DEMOD, want_var=False)
    assert_same_bits(got, want, "iterations 0, no output variance")
    assert (sentinel == -7.0).all()


@pytest.mark.parametrize("flags", [0, DEMOD], ids=["plain", "demodulated"])
def test_guided_zero_variance_plane(filt, flags):
    """kl = 2^20: any brightness difference above 2^-20 fails the colour test."""
    frame, feat, var = H.synthetic(33, 40, 22)
    var[:] = 0
    for terms in ("color", "all"):
        got, gv = check(filt, frame, feat, var, make_dn(5, TERMS[terms]), flags, f"zero variance, {terms}")
        assert (gv == 0).all()


@pytest.mark.parametrize("flags", [0, DEMOD], ids=["plain", "demodulated"])
def test_guided_nan_pixels(filt, flags):
    """One NaN variance pixel: no colour becomes NaN.  One NaN colour pixel: it stays the only
    one.  An all-NaN frame stays all NaN."""
    frame, feat, var = H.synthetic(24, 40, 4)
    v1 = var.copy()
    v1[11, 9] = np.nan
    for terms in ("all", "color", "normal"):
        got, gv = check(filt, frame, feat, v1, make_dn(5, TERMS[terms]), flags, f"NaN variance, {terms}")
        assert not np.isnan(got).any() and np.isnan(gv[11, 9])
    f1 = frame.copy()
    f1[11, 9, 2] = np.nan
    got, _ = check(filt, f1, feat, var, make_dn(5, TERMS["all"]), flags, "NaN colour")
    assert np.isnan(got[11, 9, 2]) and np.isnan(got).sum() == 1
    check(filt, f1, feat, var, make_dn(3, TERMS["normal"]), flags, "NaN colour, no colour term")
    f1[:] = np.nan
    got, _ = check(filt, f1, feat, var, make_dn(5, TERMS["all"]), flags, "all-NaN frame")
    assert np.isnan(got[:, :24]).all()


def test_guided_albedo_at_the_threshold(filt):
    """Albedo channels at 0, at a_min exactly (both left alone) and one ulp above (divided), a
    pixel whose mean albedo is at most a_min, and a NaN albedo: the kernel takes the
    restatement's branches."""
    frame, feat, var = H.synthetic(24, 24, 5)
    a_min = G.A_MIN
    above = np.nextafter(a_min, F(1.0))
    feat[5, 5, 4:7] = (0.0, a_min, above)
    feat[6, 9, 4:7] = (a_min, a_min, a_min)
    feat[7, 3, 4:7] = (above, 0.0, 0.0)
    feat[9, 9, 4:7] = (np.nan, 0.5, 0.5)
    feat[12:16, 12:16, 4:7] = 0.0
    for terms in ("none", "color", "all"):
        for iters in (1, 3):
            check(filt, frame, feat, var, make_dn(iters, TERMS[terms]), DEMOD, f"albedo threshold, {terms}, {iters}")
    plain, _ = G.guided_dn(frame, feat, var, make_dn(1, TERMS["none"]), 0)
    dem, _ = G.guided_dn(frame, feat, var, make_dn(1, TERMS["none"]), DEMOD)
    assert (plain != dem).any()


def test_guided_refusals(filt):
    frame, feat, var = H.synthetic(24, 24, 6)
    dn = make_dn(1, TERMS["all"])
    for kw in ({"inplace": True}, {"null_var": True}, {"misalign": True}, {"flags": 2}):
        with pytest.raises(z.ZrtError) as e:
            filt.run(frame, feat, var, dn, **kw)
        assert e.value.code == _ffi.ZRT_E_INVALID, kw
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(z.ZrtError) as e:
            filt.run(frame, feat, var, _ffi.Denoise(iterations=1, sigma_color=bad))
        assert e.value.code == _ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:
        filt.run(frame, feat, var, _ffi.Denoise(iterations=9, sigma_color=1.0))
    assert e.value.code == _ffi.ZRT_E_INVALID
    # the plain filter still runs on the context afterwards, and reports its own time
    want = R.atrous_dn(frame, feat, D.make_dn(2, D.TERMS["all"]))
    got = D.Filter.run(filt, frame, feat, D.make_dn(2, D.TERMS["all"]))
    assert_same_bits(got, want, "the plain filter after the guided one")


# ---- end to end -------------------------------------------------------------------------

def e2e_params():
    return z.RenderParams(32, 32, 32, V.DEPTH, sample_chunk=4)


def test_render_denoised_guided_end_to_end(scenes):
    """32 x 32, 32 spp in chunks of 4: the noisy frame is z.render's, the variance plane the
    oracle-derived one, the features the oracle's, and the output the restatement applied to
    those - with the defaults and with an explicit filter and flag."""
    _, view, cam = S.get("bubbles")
    p = e2e_params()
    plain, pst = z.render(view, cam, p)
    want_var = G.frame_variance(V.sums_of(scenes, "bubbles", p, 8), 4, 32)
    want_feat = D.expected("bubbles", scenes, 32, 32)[0]
    dn, flags = z.denoise_guided_defaults()
    rgb, noisy, feat, var, st = z.render_denoised_guided(view, cam, p)
    assert_same_bits(noisy, plain, "noisy")
    assert st["rays_processed"] == pst["rays_processed"] and st["denoise_ms"] > 0.0
    V.assert_plane(var, want_var, "variance")
    assert_same_bits(feat, want_feat, "features")
    assert_same_bits(rgb, G.guided_dn(plain, want_feat, want_var, dn, flags)[0], "rgb")
    assert (rgb != noisy).any()
    for fl in (0, DEMOD):
        dn2 = make_dn(2, TERMS["all"])
        rgb2, noisy2, _, var2, _ = z.render_denoised_guided(view, cam, p, denoise=dn2, flags=fl)
        assert_same_bits(noisy2, plain, "noisy, explicit filter")
        V.assert_plane(var2, want_var, "variance, explicit filter")
        assert_same_bits(rgb2, G.guided_dn(plain, want_feat, want_var, dn2, fl)[0], f"rgb, explicit filter, flags {fl}")


def test_render_denoised_guided_adaptive(scenes):
    """The adaptive one-shot at 32 x 32, cap 32 in chunks of 4, first level 8: the noisy frame is
    z.render_adaptive's, every tile's variance uses its own chunk count."""
    _, view, cam = S.get("bubbles")
    p = e2e_params()
    ex = A.expected_run(scenes, "bubbles", p, 8)
    assert ex.levels == [8, 16, 32]
    final = ex.samples(len(ex.steps) - 1)
    assert len(set(final.tolist())) == 2, final  # (the one decision, at 16 samples, stops some tiles)
    sums = V.sums_of(scenes, "bubbles", p, 8)
    want_var = np.zeros((32, 32), F)
    for t, (x0, x1, y0, y1) in enumerate(A.tile_boxes(p)):
        want_var[y0:y1, x0:x1] = G.frame_variance(sums[:int(final[t]) // 4], 4, 32)[y0:y1, x0:x1]
    plain, samples, pst, _ = z.render_adaptive(view, cam, p, ex.tol, 8)
    assert_same_bits(plain, ex.frames[-1], "the adaptive frame")
    dn, flags = z.denoise_guided_defaults()
    rgb, noisy, feat, var, st = z.render_denoised_guided(view, cam, p, tolerance=ex.tol, first_level=8)
    assert_same_bits(noisy, plain, "noisy (adaptive)")
    assert st["samples_processed"] == pst["samples_processed"]
    V.assert_plane(var, want_var, "variance (adaptive)")
    assert_same_bits(rgb, G.guided_dn(plain, feat, want_var, dn, flags)[0], "rgb (adaptive)")


def test_cli_denoise_variance(scenes, tmp_path):
    """zrt-raytrace 32 32 64 5 1 out.png with ZRT_DENOISE=1 and ZRT_DENOISE_VARIANCE=1 / =2: the
    PNG of the guided defaults without and with demodulation on the default chunk's two chunk
    sums; ZRT_DENOISE_NOISY the unfiltered frame; 8 spp (a quarter chunk) is refused, and
    ZRT_SAMPLE_CHUNK=4 is the remedy."""
    s = scenes(1)
    p = z.RenderParams(32, 32, 64, 5, seed=42, sample_chunk=0)
    plain, _ = z.render(s, s.camera, p)
    feat = D.expected(1, scenes, 32, 32)[0]
    var = G.frame_variance(V.sums_of(scenes, 1, p, 2), 32, 32)
    dn, _ = z.denoise_guided_defaults()
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    drop = ("ZRT_PASS_SAMPLES", "ZRT_DEVICES", "ZRT_ADAPTIVE_TOL", "ZRT_SAMPLE_CHUNK", "ZRT_DENOISE_VARIANCE")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(ZRT_DENOISE="1", ZRT_DENOISE_NOISY=str(tmp_path / "noisy.png"))

    def cli(spp, out, **extra):
        return subprocess.run([exe, "32", "32", str(spp), "5", "1", str(tmp_path / out)], env={**env, **extra},
                              capture_output=True, text=True, timeout=120)

    z.write_png(str(tmp_path / "want_noisy.png"), plain)
    outs = []
    for mode, flags in (("1", 0), ("2", DEMOD)):
        r = cli(64, f"out{mode}.png", ZRT_DENOISE_VARIANCE=mode)
        assert r.returncode == 0, r.stderr
        assert "variance-guided" in r.stderr and ("demodulated" in r.stderr) == (mode == "2")
        z.write_png(str(tmp_path / f"want{mode}.png"), G.guided_dn(plain, feat, var, dn, flags)[0])
        outs.append((tmp_path / f"out{mode}.png").read_bytes())
        assert outs[-1] == (tmp_path / f"want{mode}.png").read_bytes()
        assert (tmp_path / "noisy.png").read_bytes() == (tmp_path / "want_noisy.png").read_bytes()
    assert outs[0] != outs[1] and outs[0] != (tmp_path / "noisy.png").read_bytes()
    r = cli(8, "short.png", ZRT_DENOISE_VARIANCE="1")
    assert r.returncode != 0 and "sample_chunk" in r.stderr and not (tmp_path / "short.png").exists()
    r = cli(8, "chunk4.png", ZRT_DENOISE_VARIANCE="1", ZRT_SAMPLE_CHUNK="4")
    assert r.returncode == 0, r.stderr
    r = cli(64, "bad.png", ZRT_DENOISE_VARIANCE="3")
    assert r.returncode != 0 and "ZRT_DENOISE_VARIANCE" in r.stderr
    r = cli(64, "both.png", ZRT_DENOISE_VARIANCE="1", ZRT_PASS_SAMPLES="32")
    assert r.returncode != 0 and "ZRT_DENOISE" in r.stderr and not (tmp_path / "both.png").exists()


# ---- quality ----------------------------------------------------------------------------

@pytest.mark.parametrize("key", [1, 2, "glass-inside", "bubbles"], ids=str)
def test_guided_frame_is_closer_to_the_converged_one(scenes, key):
    """The guided defaults on a 32-spp frame (chunks of 4) at 64 x 64 lower its RMSE against the
    4096-spp frame: the condition the plain defaults were held to.  The plain default filter's
    RMSE on the same frame is printed beside it (a measurement: DESIGN.md section 5)."""
    view, cam = D.scene_of(key, scenes)
    p = z.RenderParams(64, 64, 32, 20, sample_chunk=4)
    rgb, noisy, _, _, _ = z.render_denoised_guided(view, cam, p)
    plain, noisy2, _, _ = z.render_denoised(view, cam, p)
    assert_same_bits(noisy, noisy2, "the two one-shots' noisy frames")
    ref, _ = z.render(view, cam, dataclasses.replace(p, samples_per_pixel=4096, sample_chunk=0))
    e_noisy, e_rgb, e_plain = D.rmse(noisy, ref, 64), D.rmse(rgb, ref, 64), D.rmse(plain, ref, 64)
    print(f"{key}: rmse noisy {e_noisy:.5f} guided {e_rgb:.5f} (ratio {e_rgb / e_noisy:.3f}) "
          f"plain filter {e_plain:.5f} (ratio {e_plain / e_noisy:.3f})")
    assert e_rgb < e_noisy

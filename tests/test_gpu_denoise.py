"""GPU tests of the denoiser: the first-hit feature buffers against values composed from
the oracle (tests/denoise_ref.expected_features), the a-trous filter bit for bit against
its numpy restatement (tests/denoise_ref.atrous) on synthetic buffers, the one-shot
entry point and the command-line client end to end, and the quality condition the
default sigmas were chosen under (tools/denoise_probe.py)."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

import denoise_ref as R
import shading_scenes as S

pytestmark = pytest.mark.gpu
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what=""):
    g, w = bits(got), bits(want)
    same = (g == w) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        idx = np.argwhere(~same)
        i = tuple(idx[0])
        raise AssertionError(f"{what}: {len(idx)} of {g.size} values differ, first at {i}: got {got[i]!r} "
                             f"({g[i]:#x}) want {want[i]!r} ({w[i]:#x})")


# ---- features ---------------------------------------------------------------------------

_EXPECTED = {}


def scene_of(key, scenes):
    """key: a name of shading_scenes.NAMES or a loaded scene's index -> (view, camera)."""
    if isinstance(key, int):
        s = scenes(key)
        return s.view, s.camera
    _, view, cam = S.get(key)
    return view, cam


def expected(key, scenes, w, h):
    if (key, w, h) not in _EXPECTED:
        view, cam = scene_of(key, scenes)
        _EXPECTED[(key, w, h)] = R.expected_features(O, view, cam, w, h)
    return _EXPECTED[(key, w, h)]


def gpu_features(view, cam, p):
    import torch
    ctx = z.RenderContext(view, p)
    try:
        buf = torch.full((p.height * p.width * 8,), float("nan"), dtype=torch.float32, device="cuda")
        ctx.features(cam, p, buf.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        return buf.cpu().numpy().reshape(p.height, p.width, 8).copy()
    finally:
        ctx.close()


FEATURE_CASES = [("glass-inside", 24, 24), ("bubbles", 24, 24), ("wraps", 24, 24), ("poles", 24, 24),
                 (1, 32, 32), (2, 32, 32), ("bubbles", 40, 24)]


@pytest.mark.parametrize("key,w,h", FEATURE_CASES, ids=[f"{k}-{w}x{h}" for k, w, h in FEATURE_CASES])
def test_features_equal_the_oracle(scenes, key, w, h):
    """Every traversal writes the buffer the oracle composes: normal, t, albedo and id of
    each pixel's first hit, the background on a miss, zeros outside the rendered square.
    "wraps" and "bubbles" carry the image-textured mesh (the mound's facets), "glass-inside"
    the dielectric first hit met from the back, "poles" and "wraps" every texture-wrap arm."""
    view, cam = scene_of(key, scenes)
    want, tri = expected(key, scenes, w, h)
    if key in ("wraps", "bubbles"):
        assert len(tri) >= 10  # image-textured triangles are among the first hits
    if w > h:
        assert (want[:, h:] == 0).all()
    for trav in (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE):
        p = z.RenderParams(w, h, 1, 1, traversal=trav)
        got = gpu_features(view, cam, p)
        assert_same_bits(got, want, f"{key} traversal {trav}")


def test_features_ignore_rank_and_world_size(scenes):
    view, cam = scene_of("bubbles", scenes)
    want, _ = expected("bubbles", scenes, 24, 24)
    got = gpu_features(view, cam, z.RenderParams(24, 24, 1, 1, rank=1, world_size=3))
    assert_same_bits(got, want, "rank 1 of 3")


# ---- the filter on synthetic buffers ----------------------------------------------------

def synthetic(h, w, seed):
    """Seeded noise over a two-plane normal edge (x = w / 2), a depth step (y = h / 2) and a
    miss region (the top right corner): (frame[h, w, 3], features[h, w, 8])."""
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
    return frame, f


class Filter:
    """One context and its device buffers, for many small denoise calls."""

    def __init__(self):
        _, view, _ = S.get("bubbles")
        self.ctx = z.RenderContext(view, z.RenderParams(8, 8, 1, 1))

    def run(self, frame, feat, dn, inplace=False):
        import torch
        h, w, _ = frame.shape
        p = z.RenderParams(w, h, 1, 1)
        d_in = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
        d_ft = torch.from_numpy(np.ascontiguousarray(feat)).cuda()
        d_out = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
        self.ctx.denoise(p, dn, d_in.data_ptr(), d_ft.data_ptr(), d_in.data_ptr() if inplace else d_out.data_ptr())
        ms = self.ctx.denoise_ms()
        torch.cuda.synchronize()
        assert ms >= 0.0
        return d_out.cpu().numpy()


@pytest.fixture(scope="module")
def filt():
    f = Filter()
    yield f
    f.ctx.close()


SIGMAS = (0.5, 0.25, 0.5, 0.25)  # colour, normal (|dN|^2 = 0.4 across the edge), albedo, relative depth
TERMS = {"color": (1, 0, 0, 0), "normal": (0, 1, 0, 0), "albedo": (0, 0, 1, 0), "depth": (0, 0, 0, 1),
         "all": (1, 1, 1, 1), "none": (0, 0, 0, 0)}


def make_dn(iters, on):
    s = [v if o else 0.0 for v, o in zip(SIGMAS, on)]
    return _ffi.Denoise(iterations=iters, sigma_color=s[0], sigma_normal=s[1], sigma_albedo=s[2], sigma_depth=s[3])


@pytest.mark.parametrize("h,w", [(1, 1), (24, 24), (24, 40), (70, 70)], ids=["1x1", "24x24", "40x24", "70x70"])
@pytest.mark.parametrize("terms", list(TERMS))
def test_filter_equals_the_restatement(filt, h, w, terms):
    """Iterations 1 (LDS, step 1), 3 (the first step read from memory), 5 and 8 (step 128
    exceeds the frame: the centre tap alone) - 70 x 70 crosses block and halo boundaries."""
    frame, feat = synthetic(h, w, 1000 * h + w)
    for iters in (1, 3, 5, 8):
        dn = make_dn(iters, TERMS[terms])
        got = filt.run(frame, feat, dn)
        want = R.atrous_dn(frame, feat, dn)
        assert_same_bits(got, want, f"{w}x{h} {terms} iterations {iters}")
        if terms != "none" and h > 1 and iters == 1:
            assert (got[:, :h] != frame[:, :h]).any()


def test_filter_default_iterations(filt):
    frame, feat = synthetic(24, 24, 3)
    dn0, dn5 = make_dn(0, TERMS["all"]), make_dn(5, TERMS["all"])
    assert_same_bits(filt.run(frame, feat, dn0), R.atrous_dn(frame, feat, dn5), "iterations 0")


def test_filter_one_nan_pixel(filt):
    frame, feat = synthetic(24, 40, 4)
    frame[11, 9, 2] = np.nan
    dn = make_dn(5, TERMS["all"])
    got = filt.run(frame, feat, dn)
    want = R.atrous_dn(frame, feat, dn)
    assert np.isnan(got[11, 9, 2]) and np.isnan(got).sum() == np.isnan(want).sum() == 1
    assert_same_bits(got, want, "one NaN pixel")
    # colour term off: the NaN spreads through the weighted sums, in both the same way
    dn = make_dn(3, TERMS["normal"])
    assert_same_bits(filt.run(frame, feat, dn), R.atrous_dn(frame, feat, dn), "one NaN pixel, no colour term")


def test_filter_all_nan_frame(filt):
    frame, feat = synthetic(24, 24, 5)
    frame[:] = np.nan
    got = filt.run(frame, feat, make_dn(5, TERMS["all"]))
    assert np.isnan(got).all()


def test_filter_refuses_in_place(filt):
    frame, feat = synthetic(24, 24, 6)
    with pytest.raises(z.ZrtError) as e:
        filt.run(frame, feat, make_dn(1, TERMS["all"]), inplace=True)
    assert e.value.code == _ffi.ZRT_E_INVALID


# ---- end to end -------------------------------------------------------------------------

def test_render_denoised_end_to_end(scenes):
    _, view, cam = S.get("bubbles")
    p = z.RenderParams(24, 24, 8, 6)
    rgb, noisy, feat, st = z.render_denoised(view, cam, p)
    plain, pst = z.render(view, cam, p)
    assert_same_bits(noisy, plain, "noisy")
    assert st["rays_processed"] == pst["rays_processed"] and st["denoise_ms"] > 0.0
    assert_same_bits(feat, expected("bubbles", scenes, 24, 24)[0], "features")
    assert_same_bits(rgb, R.atrous_dn(noisy, feat, z.denoise_defaults()), "rgb")
    assert (rgb != noisy).any()
    # an explicit filter
    dn = make_dn(2, TERMS["all"])
    rgb2, noisy2, feat2, _ = z.render_denoised(view, cam, p, denoise=dn)
    assert_same_bits(noisy2, plain, "noisy, explicit filter")
    assert_same_bits(rgb2, R.atrous_dn(plain, feat, dn), "rgb, explicit filter")


def test_render_denoised_adaptive(scenes):
    _, view, cam = S.get("bubbles")
    p = z.RenderParams(24, 24, 8, 6, sample_chunk=2)
    tol = 2.0  # (loose: the one decision, at 4 samples, stops most tiles)
    assert z.adapt_plan(p, tol, 2) == [2, 4, 8]
    rgb, noisy, feat, st = z.render_denoised(view, cam, p, tolerance=tol, first_level=2)
    plain, samples, pst, _ = z.render_adaptive(view, cam, p, tol, 2)
    assert samples.min() < 8  # some tile stopped early: the adaptive frame is not the plain one
    assert_same_bits(noisy, plain, "noisy (adaptive)")
    assert st["samples_processed"] == pst["samples_processed"]
    assert_same_bits(feat, expected("bubbles", scenes, 24, 24)[0], "features (adaptive)")
    assert_same_bits(rgb, R.atrous_dn(noisy, feat, z.denoise_defaults()), "rgb (adaptive)")


def test_cli_denoise(scenes, tmp_path):
    """zrt-raytrace 32 32 8 5 1 out.png with ZRT_DENOISE=1: the PNG of the default-filtered
    frame, ZRT_DENOISE_NOISY the unfiltered one; an explicit filter; refused with passes."""
    s = scenes(1)
    p = z.RenderParams(32, 32, 8, 5, seed=42, sample_chunk=0)
    plain, _ = z.render(s, s.camera, p)
    feat = expected(1, scenes, 32, 32)[0]
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    env = {k: v for k, v in os.environ.items() if k not in ("ZRT_PASS_SAMPLES", "ZRT_DEVICES", "ZRT_ADAPTIVE_TOL")}
    env.update(ZRT_DENOISE="1", ZRT_DENOISE_NOISY=str(tmp_path / "noisy.png"))
    r = subprocess.run([exe, "32", "32", "8", "5", "1", str(tmp_path / "out.png")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "  Denoise:               5 iterations" in r.stderr
    z.write_png(str(tmp_path / "want.png"), R.atrous_dn(plain, feat, z.denoise_defaults()))
    z.write_png(str(tmp_path / "want_noisy.png"), plain)
    assert (tmp_path / "out.png").read_bytes() == (tmp_path / "want.png").read_bytes()
    assert (tmp_path / "noisy.png").read_bytes() == (tmp_path / "want_noisy.png").read_bytes()
    assert (tmp_path / "out.png").read_bytes() != (tmp_path / "noisy.png").read_bytes()
    env2 = {**env, "ZRT_DENOISE": "2,0.5,0.25,0,0.125"}
    r = subprocess.run([exe, "32", "32", "8", "5", "1", str(tmp_path / "out2.png")], env=env2, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    z.write_png(str(tmp_path / "want2.png"), R.atrous(plain, feat, 2, 0.5, 0.25, 0.0, 0.125))
    assert (tmp_path / "out2.png").read_bytes() == (tmp_path / "want2.png").read_bytes()
    r = subprocess.run([exe, "32", "32", "8", "5", "1", str(tmp_path / "both.png")],
                       env={**env, "ZRT_PASS_SAMPLES": "32"}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ZRT_DENOISE" in r.stderr and not (tmp_path / "both.png").exists()


# ---- quality ----------------------------------------------------------------------------

def rmse(a, b, n):
    d = (a.astype(np.float64) - b.astype(np.float64))[:, :n]
    return float(np.sqrt((d * d).mean()))


@pytest.mark.parametrize("key", [1, 2, "glass-inside", "bubbles"], ids=str)
def test_denoised_frame_is_closer_to_the_converged_one(scenes, key):
    """The default filter on an 8-spp frame at 64 x 64 lowers its RMSE against the
    4096-spp frame (z.render, pinned to the oracle by the parity suite)."""
    view, cam = scene_of(key, scenes)
    p = z.RenderParams(64, 64, 8, 20)
    rgb, noisy, _, _ = z.render_denoised(view, cam, p)
    ref, _ = z.render(view, cam, dataclasses.replace(p, samples_per_pixel=4096))
    e_noisy, e_rgb = rmse(noisy, ref, 64), rmse(rgb, ref, 64)
    print(f"{key}: rmse noisy {e_noisy:.5f} denoised {e_rgb:.5f} ratio {e_rgb / e_noisy:.3f}")
    assert e_rgb < e_noisy

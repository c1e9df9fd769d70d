"""CPU tests of the camera-query reference (tests/camera_ref.py): the pinhole composition is
oracle_render's own frame on the square it renders, counters included; the key identity holds
at large pixel indices; a thin lens of aperture 0 is the pinhole; zrt_lens_init equals its
numpy restatement and, at focus_dist 1, zrt_camera_init's plane.  No kernel is launched."""
import numpy as np
import pytest

import camera_ref as CR
import radiance_ref as R
import shading_scenes as S
import zraytrace_amd as z
from oracle import oracle_py as O

F = np.float32
SCENES = ("wraps", "bubbles", "glass-inside")
PRNGS = [z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256]
W, H, SPP, CHUNK, DEPTH = 12, 8, 5, 2, 6
POSE = ((0.4, 1.7, -3.6), (0.1, 0.2, 0.0), (0.0, 1.0, 0.0), 40.0, 1.5)
FIELDS = ("origin", "lower_left_corner", "horizontal", "vertical", "axis_u", "axis_v", "axis_w")


def params(prng, seed=42):
    return z.RenderParams(W, H, SPP, DEPTH, seed=seed, prng=prng, sample_chunk=CHUNK)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("prng", PRNGS, ids=["xoroshiro", "xoshiro"])
def test_pinhole_composition_is_the_oracles_frame(name, prng):
    """12 x 8, 5 samples, chunk 2, depth 6: on the square x < height the composed means are
    O.render's with the real camera bit for bit, and the square's counters are its stats."""
    _, view, cam = S.get(name)
    p = params(prng)
    fr = CR.Frame(O, view, p, CR.lens_of_camera(cam), SPP)
    img, st = O.render(view, cam, p)
    got = fr.image(fr.rgb)
    assert R.same_bits(got[:, :H], img[:, :H]).all()
    assert not img[:, H:].any(), "the oracle rendered past the square"
    assert (got[:, H:] != 0).any(), "the composition does not cover the whole width"
    sq = R.info_of(fr.image(fr.counters)[:, :H].reshape(-1, len(R.COUNTERS)))
    for k in R.COUNTERS:
        assert sq[k] == st[R._STATS[k]], k
    assert sq["samples"] == H * H * SPP
    assert fr.info["samples"] == W * H * SPP
    # the prefix of a frame is the frame of fewer samples
    two = fr.prefix(2)
    img2, _ = O.render(view, cam, z.RenderParams(W, H, 2, DEPTH, seed=42, prng=prng, sample_chunk=CHUNK))
    assert R.same_bits(two.image(two.rgb)[:, :H], img2[:, :H]).all()


@pytest.mark.parametrize("prng", PRNGS, ids=["xoroshiro", "xoshiro"])
def test_key_identity_at_large_pixel_indices(prng):
    for pixel in (65534 * 65535 + 65534, (1 << 31) + 7, (1 << 32) - 1):
        for seed in (0, 42, (1 << 64) - 3):
            for s in (0, 1, 65535):
                assert R.key_of(0, 0, R.shifted_seed(seed, pixel, s)) == R.key_of(pixel, s, seed)
                assert R.key_of(pixel, s, seed) == (((pixel << 16) + s) + seed * R.GOLDEN) & R.MASK64
    # through the oracle: the last pixel of a 65535-wide row draws the composed sample's stream
    _, view, cam = S.get("wraps")
    p = z.RenderParams(65535, 3, 1, DEPTH, seed=42, prng=prng, sample_chunk=0)
    rect = (65533, 2, 2, 1)
    fr = CR.Frame(O, view, p, CR.lens_of_camera(cam), 2, rect=rect)
    assert list(fr.R) == [2 * 65535 + 65533, 2 * 65535 + 65534]
    other = CR.Frame(O, view, z.RenderParams(65535, 3, 1, DEPTH, seed=43, prng=prng), CR.lens_of_camera(cam), 2, rect=rect)
    assert not R.same_bits(fr.t, other.t).all(), "the seed does not reach the jitter"


def test_thin_lens_of_aperture_zero_is_the_pinhole():
    _, view, _ = S.get("wraps")
    p = params(0)
    pin = z.lens_init(z.ZRT_LENS_PINHOLE, *POSE)
    thin = z.lens_init(z.ZRT_LENS_THIN, *POSE, aperture=0.0, focus_dist=1.0)
    a = CR.Frame(O, view, p, pin, 3)
    b = CR.Frame(O, view, p, thin, 3)
    assert R.same_bits(a.o, b.o).all() and R.same_bits(a.t, b.t).all()
    assert R.same_bits(a.sum, b.sum).all() and a.info == b.info
    wide = CR.Frame(O, view, p, z.lens_init(z.ZRT_LENS_THIN, *POSE, aperture=0.5, focus_dist=3.0), 3)
    assert (wide.o != a.o).any(-1).all(), "a lens sample on the axis in every draw"
    assert not R.same_bits(wide.rgb, a.rgb).all(-1).all()


@pytest.mark.parametrize("kind", range(5))
def test_lens_init_equals_its_restatement(kind):
    for aperture, focus, fov in ((0.0, 1.0, 180.0), (0.3, 3.5, 120.0), (2.0, 0.25, 220.0)):
        lens = z.lens_init(kind, *POSE, aperture=aperture, focus_dist=focus, fisheye_fov=fov)
        want = CR.lens_init_np(O, kind, *POSE, aperture, focus, fov)
        assert lens.kind == kind
        for k in FIELDS:
            assert R.same_bits(CR.vec(getattr(lens, k)), want[k]).all(), (k, CR.vec(getattr(lens, k)), want[k])
        assert R.same_bits([lens.half_fov], [want["half_fov"]]).all()
        # at focus_dist 1 the plane is zrt_camera_init's (and the oracle's), whatever the aperture
        one = z.lens_init(kind, *POSE, aperture=aperture, focus_dist=1.0, fisheye_fov=fov)
        for cam in (z.camera_init(*POSE), O.camera_init(*POSE)):
            for k in FIELDS[:4]:
                assert R.same_bits(CR.vec(getattr(one, k)), CR.vec(getattr(cam, k))).all(), k


@pytest.mark.parametrize("kind", range(5))
def test_lens_from_camera_equals_its_restatement(kind):
    """Every kind, the camera's own plane (focus_dist 0) and rescaled planes, on a camera_init
    camera (plane at distance 1) and on one whose plane is neither at 1 nor square."""
    far = z.camera_init(*POSE)
    for k in ("lower_left_corner", "horizontal", "vertical"):  # the plane pushed out 2.5 times
        for c in "xyz":
            o = getattr(far.origin, c)
            setattr(getattr(far, k), c, float(F(2.5) * F(getattr(getattr(far, k), c) - (o if k == "lower_left_corner" else 0)))
                    + (o if k == "lower_left_corner" else 0.0))
    for cam in (z.camera_init(*POSE), S.get("glass-inside")[2], far):
        for aperture, focus, fov in ((0.0, 0.0, 180.0), (0.3, 3.5, 120.0), (2.0, 0.25, 220.0), (0.05, 1.0, 150.0)):
            lens = z.lens_from_camera(kind, cam, aperture=aperture, focus_dist=focus, fisheye_fov=fov)
            want = CR.lens_from_camera_np(kind, cam, aperture, focus, fov)
            assert lens.kind == kind
            for k in FIELDS:
                assert R.same_bits(CR.vec(getattr(lens, k)), want[k]).all(), (k, CR.vec(getattr(lens, k)), want[k])
            assert R.same_bits([lens.half_fov], [want["half_fov"]]).all()
            if focus == 0.0:  # the camera's own plane, bit for bit
                for k in FIELDS[:4]:
                    assert R.same_bits(CR.vec(getattr(lens, k)), CR.vec(getattr(cam, k))).all(), k
            else:  # the rescaled plane's centre lies focus_dist along the axis (a check of the restatement itself)
                centre = CR.vec(lens.lower_left_corner) + 0.5 * CR.vec(lens.horizontal) + 0.5 * CR.vec(lens.vertical)
                d = centre.astype(np.float64) - CR.vec(cam.origin)
                assert abs(np.linalg.norm(d) - focus) < 1e-5 * max(1.0, focus)
                assert np.allclose(d / np.linalg.norm(d), CR.vec(lens.axis_w), atol=1e-5)
                ratio = np.linalg.norm(CR.vec(lens.horizontal)) / np.linalg.norm(CR.vec(cam.horizontal))
                assert abs(ratio - np.linalg.norm(CR.vec(lens.vertical)) / np.linalg.norm(CR.vec(cam.vertical))) < 1e-5
    with pytest.raises(z.ZrtError):
        z.lens_from_camera(5, far)


def test_lens_init_refusals():
    for bad in (lambda: z.lens_init(5, *POSE), lambda: z.lens_init(4, *POSE, fisheye_fov=0.0),
                lambda: z.lens_init(4, *POSE, fisheye_fov=-10.0),
                lambda: z.lens_init(1, *POSE, aperture=float("inf")),
                lambda: z.lens_init(0, POSE[0], POSE[0], *POSE[2:]),  # look_from == look_at: a NaN basis
                lambda: z.lens_init(2, *POSE, focus_dist=float("nan"))):
        with pytest.raises(z.ZrtError) as e:
            bad()
        assert e.value.code == z._ffi.ZRT_E_INVALID

"""GPU tests of the temporal accumulation: zrt_ctx_temporal bit for bit against its numpy
restatement (tests/temporal_ref.Temporal) - colour, variance and history length - on
synthetic sequences and on rendered ones, the one-shot entry point against the same
composition done call by call, the command-line client, and the quality condition the
defaults were chosen under (tools/temporal_probe.py)."""
import dataclasses
import json
import os
import subprocess

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi

import shading_scenes as S
import temporal_ref as T
import test_gpu_denoise as D
import test_temporal_host as TH

pytestmark = pytest.mark.gpu
F = np.float32
DEMOD = z.ZRT_TA_DEMODULATE
SENTINEL, LEN_SENTINEL = -7.0, 7777

assert_same_bits = D.assert_same_bits


class Runner:
    """One context, and a restatement fed the same calls."""

    def __init__(self):
        _, view, _ = S.get("bubbles")
        self.ctx = z.RenderContext(view, z.RenderParams(8, 8, 1, 1))
        self.ref = T.Temporal()

    def reset(self):
        self.ctx.temporal_reset()
        self.ref.reset()

    def gpu(self, cam, frame, feat, var, tp, want_var=True, want_len=True, inplace=False, null_var=False,
            misalign=False):
        import torch
        h, w, _ = frame.shape
        p = z.RenderParams(w, h, 1, 1)
        d_in = torch.from_numpy(np.ascontiguousarray(frame)).cuda()
        d_ft = torch.zeros(h * w * 8 + 4, dtype=torch.float32, device="cuda")
        d_ft[:h * w * 8] = torch.from_numpy(np.ascontiguousarray(feat)).cuda().reshape(-1)
        d_var = torch.from_numpy(np.ascontiguousarray(var)).cuda()
        d_out = torch.full((h, w, 3), SENTINEL, dtype=torch.float32, device="cuda")
        d_ov = torch.full((h, w), SENTINEL, dtype=torch.float32, device="cuda")
        d_ol = torch.full((h, w), LEN_SENTINEL, dtype=torch.int32, device="cuda")
        self.ctx.temporal(T.cam_struct(cam), p, tp, d_in.data_ptr(), d_ft.data_ptr() + (4 if misalign else 0),
                          0 if null_var else d_var.data_ptr(), d_in.data_ptr() if inplace else d_out.data_ptr(),
                          d_ov.data_ptr() if want_var else 0, d_ol.data_ptr() if want_len else 0)
        ms = self.ctx.temporal_ms()
        torch.cuda.synchronize()
        assert ms >= 0.0
        return d_out.cpu().numpy(), d_ov.cpu().numpy(), d_ol.cpu().numpy().astype(np.uint32)

    def step(self, cam, frame, feat, var, tp, what):
        """One frame on both sides, compared bit for bit; the outputs."""
        got = self.gpu(cam, frame, feat, var, tp)
        want = self.ref.step_tp(cam, frame, feat, var, tp)
        assert_same_bits(got[0], want[0], what)
        assert_same_bits(got[1], want[1], what + " (variance)")
        assert (got[2] == want[2]).all(), what + " (length)"
        return got


@pytest.fixture(scope="module")
def run():
    r = Runner()
    yield r
    r.ctx.close()


SIGMAS = (0.25, 0.25)  # normal, relative depth: H.synthetic's two planes and its depth step fail them
TERMS = {"both": (True, True), "normal": (True, False), "depth": (False, True), "none": (False, False)}


def make_tp(on=(True, True), alpha_min=0.0, max_history=8, flags=0):
    return _ffi.Temporal(alpha_min=alpha_min, max_history=max_history, sigma_normal=SIGMAS[0] if on[0] else 0.0,
                         sigma_depth=SIGMAS[1] if on[1] else 0.0, flags=flags)


def base_camera(h, w):
    return T.cam_array(TH.camera((0.0, 0.0, 5.0), (0.0, 0.0, 0.0), vfov=40.0, aspect=w / h))


def truck(cam, f, g=0.0):
    """The camera moved sideways by f horizontals (the command-line client's rule, f32), and
    up by g verticals."""
    c = cam.copy()
    c[0] = cam[0] + F(f) * cam[2]
    c[1] = cam[1] + F(f) * cam[2]
    if g:
        c[0] = c[0] + F(g) * cam[3]
        c[1] = c[1] + F(g) * cam[3]
    return c


def cameras(case, h, w):
    """Three cameras.  H.synthetic's depths are 2 .. 5.2 and the viewport lies at distance 1, so
    a truck of f horizontals shifts a pixel by f * w / depth pixels: "small" stays below one pixel
    at w = 70, "large" moves the near half by a quarter of the frame - both also upwards, across
    the depth step as well as the normal edge; "turned" looks back past 90 degrees
    in frame 1, so frame 1's points lie behind frame 0's camera or beside its view, and the same
    holds for frame 2, which is frame 0's camera again."""
    c0 = base_camera(h, w)
    if case == "static":
        return [c0, c0, c0]
    if case == "small":
        return [c0, truck(c0, 0.01, 0.008), truck(c0, 0.02, 0.016)]
    if case == "large":
        return [c0, truck(c0, 0.5, 0.3), truck(c0, 1.0, 0.6)]
    back = T.cam_array(TH.camera((0.0, 0.0, 5.0), (4.9, 0.0, 5.9), vfov=40.0, aspect=w / h))  # ~100 degrees round
    return [c0, back, c0]


SIZES = [(1, 1), (8, 8), (33, 40), (70, 70)]


@pytest.mark.parametrize("case", ["static", "small", "large", "turned"])
@pytest.mark.parametrize("h,w", SIZES, ids=["1x1", "8x8", "40x33", "70x70"])
def test_temporal_equals_the_restatement(run, h, w, case):
    """Three frames per sequence, each term alone, both, none, without and with demodulation;
    40 x 33 has columns outside D, 70 x 70 crosses block boundaries.  The counters of the
    restatement show that the moving cases take the branches they are here for."""
    feat, seq = TH.sequence(h, w, 1000 * h + w, 3)
    cams = cameras(case, h, w)
    hit = int((np.ascontiguousarray(feat[:, :h, 7]).view(np.uint32) != 0).sum())
    seen = dict(behind=0, offscreen=0, rejected_normal=0, rejected_depth=0, partial=0)
    for terms, on in TERMS.items():
        for flags in (0, DEMOD):
            run.reset()
            for k, (frame, var) in enumerate(seq):
                _, _, gl = run.step(cams[k], frame, feat, var, make_tp(on, flags=flags),
                                    f"{w}x{h} {case} {terms} flags {flags} frame {k}")
                last = run.ref.last
                assert last["history"] == (k > 0) and last["static"] == (k > 0 and case == "static")
                for key in ("behind", "offscreen", "rejected_normal", "rejected_depth"):
                    seen[key] += last[key]
                seen["partial"] += int(0 < last["blended"] < hit)
                if w > h:
                    assert (gl[:, h:] == 0).all()
            if case == "static":
                assert (gl[:, :h].max() == 3) and last["blended"] == hit
    if h >= 8 and case == "large":  # (below one pixel of motion a pixel is among its own taps)
        assert seen["partial"] > 0  # some pixels with len 1 beside some with len > 1
        assert seen["offscreen"] > 0
    if h >= 33 and case in ("small", "large"):
        assert seen["rejected_normal"] > 0 and seen["rejected_depth"] > 0
    if h >= 8 and case == "turned":
        assert seen["behind"] > 0


@pytest.mark.parametrize("alpha_min,max_history", [(0.0, 8), (1.0, 8), (0.3, 8), (0.0, 1), (0.0, 2), (0.0, 0)])
def test_temporal_blend_edges(run, alpha_min, max_history):
    """alpha_min 0 and 1, a clamp in between, max_history 1, 2 and the default over five frames."""
    feat, seq = TH.sequence(33, 40, 77, 5)
    cams = cameras("small", 33, 40)
    cams = cams + [truck(cams[0], 0.03), truck(cams[0], 0.04)]
    run.reset()
    for k, (frame, var) in enumerate(seq):
        got, gv, gl = run.step(cams[k], frame, feat, var, make_tp(alpha_min=alpha_min, max_history=max_history),
                               f"alpha_min {alpha_min} max_history {max_history} frame {k}")
        if alpha_min == 1.0 or max_history == 1:
            assert_same_bits(got, frame, "the input passes through")
        assert gl.max() == min(k + 1, max_history or T.DEFAULT_HISTORY)


@pytest.mark.parametrize("flags", [0, DEMOD], ids=["plain", "demodulated"])
def test_temporal_nan_pixels(run, flags):
    """A NaN pixel in frame 2's colour and one in its variance: each is alone in frame 2's
    output and gone from frame 3, whose pixels skip those history entries; then an all-NaN
    frame, after which every pixel starts over."""
    feat, seq = TH.sequence(24, 40, 4, 4)
    cams = cameras("small", 24, 40) + [truck(base_camera(24, 40), 0.03)]
    tp = make_tp(flags=flags)
    run.reset()
    run.step(cams[0], seq[0][0], feat, seq[0][1], tp, "frame 1")
    f1, v1 = seq[1][0].copy(), seq[1][1].copy()
    f1[11, 9, 2] = np.nan
    v1[5, 3] = np.nan
    got, gv, _ = run.step(cams[1], f1, feat, v1, tp, "frame 2, a NaN colour and a NaN variance")
    assert np.isnan(got[11, 9, 2]) and np.isnan(got).sum() == 1 and np.isnan(gv[5, 3]) and np.isnan(gv).sum() == 1
    got, gv, gl = run.step(cams[2], seq[2][0], feat, seq[2][1], tp, "frame 3")
    assert not np.isnan(got).any() and not np.isnan(gv).any() and run.ref.last["rejected_nan"] > 0
    f3 = seq[3][0].copy()
    f3[:] = np.nan
    got, _, _ = run.step(cams[3], f3, feat, seq[3][1], tp, "an all-NaN frame")
    assert np.isnan(got[:, :24]).all()
    got, _, gl = run.step(cams[3], seq[0][0], feat, seq[0][1], tp, "the frame after it")
    assert not np.isnan(got).any() and gl.max() == 1


def test_temporal_albedo_at_the_threshold(run):
    """Albedo channels at 0, at a_min exactly (both left alone) and one ulp above (divided), a
    pixel whose mean albedo is at most a_min, a NaN albedo: the kernel takes the restatement's
    branches; and the flag changes the result."""
    feat, seq = TH.sequence(24, 24, 5, 3)
    a_min = T.A_MIN
    above = np.nextafter(a_min, F(1.0))
    feat[5, 5, 4:7] = (0.0, a_min, above)
    feat[6, 9, 4:7] = (a_min, a_min, a_min)
    feat[7, 3, 4:7] = (above, 0.0, 0.0)
    feat[9, 9, 4:7] = (np.nan, 0.5, 0.5)
    feat[12:16, 12:16, 4:7] = 0.0
    cams = cameras("small", 24, 24)
    outs = {}
    for flags in (0, DEMOD):
        run.reset()
        for k, (frame, var) in enumerate(seq):
            outs[flags] = run.step(cams[k], frame, feat, var, make_tp(flags=flags), f"albedo threshold, flags {flags}")
    assert (outs[0][0] != outs[DEMOD][0]).any()


def test_temporal_reset_size_and_flag_changes(run):
    """zrt_ctx_temporal_reset, a size change and a change of ZRT_TA_DEMODULATE between frames
    each make the next frame a first frame; the size change reallocates the state."""
    feat, seq = TH.sequence(24, 24, 6, 3)
    small_feat, small_seq = TH.sequence(8, 12, 6, 1)
    cams = cameras("small", 24, 24)
    tp = make_tp()
    for how in ("reset", "size", "flag"):
        run.reset()
        _, _, gl = run.step(cams[0], seq[0][0], feat, seq[0][1], tp, how)
        _, _, gl = run.step(cams[1], seq[1][0], feat, seq[1][1], tp, how)
        assert gl.max() == 2
        if how == "reset":
            run.reset()
        elif how == "size":
            run.step(base_camera(8, 12), small_seq[0][0], small_feat, small_seq[0][1], tp, "the other size")
        got, _, gl = run.step(cams[2], seq[2][0], feat, seq[2][1], make_tp(flags=DEMOD if how == "flag" else 0), how)
        assert gl.max() == 1, how
        if how != "flag":  # (demodulated and remodulated, a pixel need not come back bit for bit)
            assert_same_bits(got, seq[2][0], how)


def test_temporal_null_outputs_and_refusals(run):
    feat, seq = TH.sequence(24, 24, 7, 2)
    cam = base_camera(24, 24)
    tp = make_tp()
    run.reset()
    run.step(cam, seq[0][0], feat, seq[0][1], tp, "frame 1")
    want = run.ref.step_tp(cam, seq[1][0], feat, seq[1][1], tp)
    got, sv, sl = run.gpu(cam, seq[1][0], feat, seq[1][1], tp, want_var=False, want_len=False)
    assert_same_bits(got, want[0], "no output variance, no output length")
    assert (sv == SENTINEL).all() and (sl == LEN_SENTINEL).all()
    for kw in ({"inplace": True}, {"null_var": True}, {"misalign": True}):
        with pytest.raises(z.ZrtError) as e:
            run.gpu(cam, seq[0][0], feat, seq[0][1], tp, **kw)
        assert e.value.code == _ffi.ZRT_E_INVALID, kw
    for bad in (_ffi.Temporal(alpha_min=1.5, max_history=4), _ffi.Temporal(alpha_min=0.5, max_history=65536),
                _ffi.Temporal(alpha_min=0.5, sigma_depth=float("nan")), _ffi.Temporal(alpha_min=0.5, flags=2)):
        with pytest.raises(z.ZrtError) as e:
            run.gpu(cam, seq[0][0], feat, seq[0][1], bad)
        assert e.value.code == _ffi.ZRT_E_INVALID
    # a refused call leaves the state alone: the next frame continues the sequence
    _, _, gl = run.step(cam, seq[0][0], feat, seq[0][1], tp, "the frame after the refusals")
    assert gl.max() == 3


# ---- end to end -------------------------------------------------------------------------

E2E = [("bubbles", z.ZRT_PRNG_XOROSHIRO128), ("bubbles", z.ZRT_PRNG_XOSHIRO256), (2, z.ZRT_PRNG_XOROSHIRO128),
       (2, z.ZRT_PRNG_XOSHIRO256)]


def rendered_inputs(view, cam, p):
    """(noisy frame, features, variance plane) of one frame, from the existing one-shot."""
    _, noisy, feat, var, _ = z.render_denoised_guided(view, T.cam_struct(cam), p)
    return noisy, feat, var


@pytest.mark.parametrize("key,prng", E2E, ids=[f"{k}-prng{r}" for k, r in E2E])
def test_render_temporal_end_to_end(scenes, run, key, prng):
    """24 x 24, 8 spp in chunks of 4, two cameras: zrt_ctx_temporal on the frames, variance planes
    and features the existing calls produce equals the restatement on them, and
    zrt_render_temporal's per-frame outputs equal the guided filter applied, call by call, to
    those outputs."""
    import torch
    view, cam0 = D.scene_of(key, scenes)
    cam0 = T.cam_array(cam0)
    cams = [cam0, truck(cam0, 0.05)]
    p = z.RenderParams(24, 24, 8, 5, sample_chunk=4, prng=prng)
    tp = z.temporal_defaults()
    dn, dn_flags = z.denoise_guided_defaults()
    want = []
    run.reset()
    for k, cam in enumerate(cams):
        frame, feat, var = rendered_inputs(view, cam, dataclasses.replace(p, seed=p.seed + k))
        acc, accv, gl = run.step(cam, frame, feat, var, tp, f"{key} frame {k}")
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (acc, feat, accv)]
        d_out = torch.zeros((24, 24, 3), dtype=torch.float32, device="cuda")
        run.ctx.denoise_guided(p, dn, dn_flags, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_out.data_ptr())
        run.ctx.denoise_ms()
        torch.cuda.synchronize()
        want.append(d_out.cpu().numpy())
    assert gl.max() == 2 and (acc != frame).any()
    frames = []
    last, st = z.render_temporal(view, [T.cam_struct(c) for c in cams], p,
                                 on_frame=lambda rgb, k: frames.append((k, rgb)) and False)
    assert [k for k, _ in frames] == [0, 1] and st["samples_processed"] == 24 * 24 * 8
    for k, rgb in frames:
        assert_same_bits(rgb, want[k], f"{key} one-shot frame {k}")
    assert_same_bits(last, want[-1], "the one-shot's last frame")
    quiet, _ = z.render_temporal(view, [T.cam_struct(c) for c in cams], p)
    assert_same_bits(quiet, want[-1], "the one-shot without a callback")


def test_cli_temporal(scenes, tmp_path):
    """ZRT_TEMPORAL_FRAMES=3 ZRT_TEMPORAL_TRUCK=0.05 zrt-raytrace 24 24 8 5 2 out.png: the PNG of
    the one-shot's last frame over the trucked cameras; a static sequence without the truck;
    refused beside the other modes."""
    s = scenes(2)
    cam0 = T.cam_array(s.camera)
    p = z.RenderParams(24, 24, 8, 5, seed=42, sample_chunk=4)
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    drop = ("ZRT_PASS_SAMPLES", "ZRT_DEVICES", "ZRT_ADAPTIVE_TOL", "ZRT_SAMPLE_CHUNK", "ZRT_DENOISE",
            "ZRT_DENOISE_VARIANCE", "ZRT_TEMPORAL_TRUCK")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env.update(ZRT_TEMPORAL_FRAMES="3", ZRT_SAMPLE_CHUNK="4")

    def cli(out, **extra):
        return subprocess.run([exe, "24", "24", "8", "5", "2", str(tmp_path / out)], env={**env, **extra},
                              capture_output=True, text=True, timeout=120)

    outs = []
    for delta in (0.05, 0.0):
        cams = [T.cam_struct(truck(cam0, F(k) * F(delta))) for k in range(3)]
        want, _ = z.render_temporal(s, cams, p)
        z.write_png(str(tmp_path / "want.png"), want)
        r = cli("out.png", **({"ZRT_TEMPORAL_TRUCK": str(delta)} if delta else {}))
        assert r.returncode == 0, r.stderr
        assert r.stderr.count("Frame: ") == 3 and "Temporal:" in r.stderr
        outs.append((tmp_path / "out.png").read_bytes())
        assert outs[-1] == (tmp_path / "want.png").read_bytes(), delta
    assert outs[0] != outs[1]
    for extra in ({"ZRT_DENOISE": "1"}, {"ZRT_PASS_SAMPLES": "4"}, {"ZRT_ADAPTIVE_TOL": "0.1"}):
        r = cli("both.png", **extra)
        assert r.returncode != 0 and "ZRT_TEMPORAL_FRAMES" in r.stderr and not (tmp_path / "both.png").exists()
    r = cli("zero.png", ZRT_TEMPORAL_FRAMES="0")
    assert r.returncode != 0 and "ZRT_TEMPORAL_FRAMES" in r.stderr
    r = cli("ragged.png", ZRT_SAMPLE_CHUNK="8")
    assert r.returncode != 0 and "sample_chunk" in r.stderr


# ---- quality ----------------------------------------------------------------------------

QUALITY = os.path.join(z.REPO, "profiles", "r12", "temporal", "quality.json")
KEYS = [1, 2, "glass-inside", "bubbles"]


def sequence_rmse(view, cam0, delta, frames=8):
    """tools/temporal_probe.py's sequence at 64 x 64, 32 spp in chunks of 4, at the defaults:
    (RMSE of the last frame after temporal + guided, after the guided filter alone) against
    4096 spp at the last camera."""
    cam0 = T.cam_array(cam0)
    cams = [truck(cam0, F(k) * F(delta)) for k in range(frames)]
    p = z.RenderParams(64, 64, 32, 20, sample_chunk=4)
    both, _ = z.render_temporal(view, [T.cam_struct(c) for c in cams], p)
    last = T.cam_struct(cams[-1])
    alone, _, _, _, _ = z.render_denoised_guided(view, last, dataclasses.replace(p, seed=p.seed + frames - 1))
    ref, _ = z.render(view, last, dataclasses.replace(p, samples_per_pixel=4096, sample_chunk=0))
    return D.rmse(both, ref, 64), D.rmse(alone, ref, 64)


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_static_sequence_beats_the_guided_filter_alone(scenes, key):
    """Eight static frames hold eight times the samples of the last one: after temporal +
    guided the last frame is closer to the converged one than after the guided filter alone."""
    view, cam = D.scene_of(key, scenes)
    e_both, e_alone = sequence_rmse(view, cam, 0.0)
    print(f"{key}: static rmse temporal + guided {e_both:.5f} guided alone {e_alone:.5f} (ratio {e_both / e_alone:.3f})")
    assert e_both < e_alone


@pytest.mark.parametrize("key", KEYS, ids=str)
def test_truck_sequence_keeps_the_recorded_ratio(scenes, key):
    """The truck sequences' ratios are what the probe measured (a scene seen through mirrors or
    glass may get worse under motion: DESIGN.md section 5); they must not get worse by more
    than the probe's own spread over three base seeds, which it records beside each."""
    with open(QUALITY) as f:
        rec = json.load(f)
    view, cam = D.scene_of(key, scenes)
    e_both, e_alone = sequence_rmse(view, cam, rec["truck_delta"])
    ratio = e_both / e_alone
    want, spread = rec["scenes"][str(key)]["truck"]["ratio"], rec["scenes"][str(key)]["truck"]["spread"]
    print(f"{key}: truck rmse temporal + guided {e_both:.5f} guided alone {e_alone:.5f} (ratio {ratio:.3f}, "
          f"recorded {want:.3f}, spread {spread:.3f})")
    assert ratio <= want + spread

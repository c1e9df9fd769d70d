"""GPU tests of the camera queries (zrt.h "camera queries"): frames through device-generated
lens rays on a resident context, bit for bit against tests/camera_ref.py (composed from
oracle_render alone, one sample at a time).

1. the pinhole: sums, means and counters equal the reference on every traversal and on the
   surface list, both PRNGs, over whole, ragged and single chunks at depths 0, 1, 2 and 12;
   on the square the render covers they equal oracle_render's and the context's own frame;
2. thin lens, orthographic, equirectangular and fisheye; 3. rectangles, the block loop and
   the rounds; 4. accumulation; 5. the device error convention; 6. no interference with runs
   and streams; 7. refusals on a context; 8. the one-shot call, the wrappers and the CLI.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import camera_ref as CR
import radiance_ref as R
import shading_scenes as S
import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

pytestmark = pytest.mark.gpu
F = np.float32
TRAVERSALS = [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE]
PRNGS = [z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256]
PRNG_IDS = ["xoroshiro", "xoshiro"]
W, H, CHUNK = 24, 16, 4
# (samples, max_depth) at sample_chunk 4, as tests/test_gpu_radiance.py
CASES = [(1, 0), (3, 1), (4, 2), (5, 12), (9, 12)]
MOST = {0: 1, 1: 3, 2: 4, 12: 9}  # the most samples a case takes at each depth: one reference per depth
FILL = -7.5  # what the frame buffers hold before a call, and keep outside the rectangle and past the frame
SCENES = ("wraps", "glass-inside")
# look_from, look_at, vup, vfov, aspect of the lens models' poses; the equirect ones stand inside the scene
POSES = {"wraps": ((0.3, 1.6, -3.4), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), 38.0, 1.5),
         "glass-inside": ((1.6, 2.1, -2.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 1.5)}
INSIDE = {"wraps": (0.1, 1.2, -0.9), "glass-inside": (1.6, 1.8, -2.2)}
MODELS = ("thin", "ortho", "equirect", "fisheye")
STAT_KEYS = ("rays_processed", "reflections", "background_hits", "recursion_depth_hits", "samples_processed",
             "pixels_processed")


def cparams(prng=0, depth=6, trav=z.ZRT_TRAVERSAL_FAST, bvh=True, chunk=CHUNK, seed=42, w=W, h=H, spp=1):
    return z.RenderParams(w, h, spp, depth, bounded_volume_hierarchy=bvh, seed=seed, prng=prng, traversal=trav,
                          sample_chunk=chunk)


@functools.lru_cache(maxsize=None)
def lens_of(name, model):
    pose = POSES[name]
    if model == "pinhole":  # the scene's own camera: the frame oracle_render and the context render
        return CR.lens_of_camera(S.get(name)[2])
    if model == "thin":
        return z.lens_init(z.ZRT_LENS_THIN, *pose, aperture=0.8, focus_dist=3.5)
    if model == "ortho":
        return z.lens_init(z.ZRT_LENS_ORTHO, pose[0], pose[1], pose[2], 100.0, pose[4])
    if model == "equirect":
        return z.lens_init(z.ZRT_LENS_EQUIRECT, INSIDE[name], *pose[1:])
    assert model == "fisheye"
    return z.lens_init(z.ZRT_LENS_FISHEYE, *pose, fisheye_fov=180.0)


@functools.lru_cache(maxsize=None)
def ref_most(name, model, prng, depth, bvh=True, w=W, h=H, most=None):
    """The reference frame of (scene, model, params) at the most samples any test takes of it."""
    return CR.Frame(O, S.get(name)[1], cparams(prng, depth, bvh=bvh, w=w, h=h), lens_of(name, model), most or MOST[depth])


def ref(name, model, prng, n_samples, depth, bvh=True, **kw):
    return ref_most(name, model, prng, depth, bvh, **kw).prefix(n_samples)


_CTX = {}


def ctx_of(name, bvh=True):
    if (name, bvh) not in _CTX:
        _CTX[name, bvh] = z.RenderContext(S.get(name)[1], cparams(bvh=bvh))
    return _CTX[name, bvh]


def run(ctx, p, lens, n_samples, rect=None, first_sample=0, into=None, accumulate=False, stream=0, sync=True):
    """One zrt_ctx_camera call: (sum float32[w h, 4], rgb float32[w h, 3], info).  The buffers
    hold FILL (or `into`: an earlier call's (sum, rgb)) and are 16 entries longer than the frame."""
    import torch
    n = p.width * p.height
    s = torch.full((n + 16, 4), FILL, dtype=torch.float32, device="cuda")
    c = torch.full((n + 16, 3), FILL, dtype=torch.float32, device="cuda")
    if into is not None:
        s[:n] = torch.from_numpy(np.ascontiguousarray(into[0], F)).cuda()
        c[:n] = torch.from_numpy(np.ascontiguousarray(into[1], F)).cuda()
    torch.cuda.synchronize()  # (the fills ran on torch's current stream)
    q = z.camera_query(*(rect or (0, 0, p.width, p.height)), n_samples, first_sample,
                       z.ZRT_CQ_ACCUMULATE if accumulate else 0)
    ctx.camera(p, lens, q, s.data_ptr(), c.data_ptr(), stream)
    if sync:
        ctx.sync()
    torch.cuda.synchronize()
    sh, ch = s.cpu().numpy(), c.cpu().numpy()
    assert (sh[n:] == F(FILL)).all() and (ch[n:] == F(FILL)).all(), "a query wrote past the frame"
    return sh[:n], ch[:n], (ctx.camera_info() if sync else None)


def assert_bits(got, want, what):
    bad = ~R.same_bits(got, want)
    if bad.any():
        i = int(np.argmax(bad.reshape(len(bad), -1).any(-1)))
        raise AssertionError(f"{what}: {int(bad.reshape(len(bad), -1).any(-1).sum())} of {len(got)} pixels differ, "
                             f"first {i}: {got[i]} != {want[i]}")


def assert_info(info, want, what):
    for k in R.COUNTERS:
        assert info[k] == want[k], f"{what}: {k} {info[k]} != {want[k]}"
    assert info["rays"] == info["samples"] + info["reflections"] - info["recursion_depth_hits"]
    assert info["kernel_ms"] > 0


def check(got, fr, what, outside=FILL):
    """A call's outputs against the reference of its rectangle; the other pixels hold `outside`."""
    s, c, info = got
    assert_bits(s[fr.R], fr.sum, what + ": sum")
    assert_bits(c[fr.R], fr.rgb, what + ": rgb")
    assert_info(info, fr.info, what)
    rest = np.ones(len(s), bool)
    rest[fr.R] = False
    assert (s[rest] == F(outside)).all() and (c[rest] == F(outside)).all(), what + ": a pixel outside the rectangle changed"


def rendered(ctx, cam, p):
    """zrt_ctx_render_tiles' assembled frame: float32[h, w, 3]."""
    import torch
    tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
    frame = torch.zeros(p.width * p.height * 3, dtype=torch.float32, device="cuda")
    ctx.render_tiles(cam, p, tiles.data_ptr())
    ctx.assemble(p, tiles.data_ptr(), frame.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()
    return frame.cpu().numpy().reshape(p.height, p.width, 3)


# ---- 1. the pinhole ------------------------------------------------------------------------

@pytest.mark.parametrize("bvh", [True, False], ids=["bvh", "list"])
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("prng", PRNGS, ids=PRNG_IDS)
@pytest.mark.parametrize("n_samples,depth", CASES)
def test_pinhole_equals_the_reference_and_the_render(name, prng, n_samples, depth, bvh):
    """Every traversal over the BVH; bounded_volume_hierarchy = 0: the surface list in the
    reference's order, whatever the traversal asked for (all three are asked)."""
    fr = ref(name, "pinhole", prng, n_samples, depth, bvh=bvh)
    cam, lens, ctx = S.get(name)[2], lens_of(name, "pinhole"), ctx_of(name, bvh)
    want, _ = O.render(S.get(name)[1], cam, cparams(prng, depth, bvh=bvh, spp=n_samples))
    assert_bits(fr.image(fr.rgb)[:, :H].reshape(-1, 3), want[:, :H].reshape(-1, 3), "the reference against oracle_render")
    for trav in TRAVERSALS:
        p = cparams(prng, depth, trav, bvh=bvh, spp=n_samples)
        got = run(ctx, p, lens, n_samples)
        check(got, fr, f"{name}, bvh {bvh}, traversal {trav}")
        frame = got[1].reshape(H, W, 3)
        assert_bits(frame[:, :H].reshape(-1, 3), want[:, :H].reshape(-1, 3), f"traversal {trav}: oracle_render's square")
        assert_bits(frame[:, :H].reshape(-1, 3), rendered(ctx, cam, p)[:, :H].reshape(-1, 3),
                    f"traversal {trav}: the context's own frame")
    if depth == 12:  # (inside the glass sphere shallow paths end black)
        assert fr.image(fr.rgb)[:, H:].any(), "nothing past the square"


# ---- 2. the other models -------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("prng", PRNGS, ids=PRNG_IDS)
def test_lens_models_equal_the_reference(name, model, prng):
    fr = ref_most(name, model, prng, 12, most=5)
    assert len(np.unique(fr.rgb, axis=0)) > W * H // 4, "a flat picture"
    if model == "thin":  # a kernel that ignores the lens cannot pass: the lens moves most pixels
        pin = CR.Frame(O, S.get(name)[1], cparams(prng, 12), z.lens_init(z.ZRT_LENS_PINHOLE, *POSES[name], focus_dist=3.5), 5)
        assert R.same_bits(pin.t, fr.t).all() and not R.same_bits(pin.o, fr.o).all(-1).any()
        assert int((~R.same_bits(pin.rgb, fr.rgb).all(-1)).sum()) >= W * H * 3 // 4
    if model == "equirect":  # every direction: rays leave through the top and the bottom rows
        d = fr.t - fr.o
        assert d[..., 1].min() < -0.9 and d[..., 1].max() > 0.9
    if model == "fisheye":  # 180 degrees: the corners look behind the image circle's rim
        assert ((fr.t - fr.o) @ CR.vec(lens_of(name, model).axis_w)).min() < 0
    for trav in TRAVERSALS:
        check(run(ctx_of(name), cparams(prng, 12, trav), lens_of(name, model), 5), fr, f"{name}, {model}, traversal {trav}")


# ---- 3. rectangles, the block loop and the rounds ------------------------------------------

def sub(fr, rect):
    """The reference of a rectangle of a frame's reference: (R, sum, rgb, info)."""
    _, _, Rs = CR.pixels_of(fr.p.width, rect)
    at = {int(r): i for i, r in enumerate(fr.R)}
    idx = np.array([at[int(r)] for r in Rs])
    out = type("Sub", (), {})()
    out.R, out.sum, out.rgb, out.info = Rs, fr.sum[idx], fr.rgb[idx], R.info_of(fr.counters[idx])
    return out


@pytest.mark.parametrize("trav", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY], ids=["fast", "binary"])
def test_rectangles(trav):
    name, model = "wraps", "fisheye"
    fr = ref_most(name, model, 0, 12, most=5)
    ctx, lens, p = ctx_of(name), lens_of(name, model), cparams(0, 12, trav)
    whole = run(ctx, p, lens, 5)
    check(whole, fr, "the frame")
    for rect in [(3, 5, 13, 9), (23, 15, 1, 1), (0, 0, 1, 1), (7, 0, 2, 16), (16, 8, 8, 8)]:
        check(run(ctx, p, lens, 5, rect), sub(fr, rect), f"rectangle {rect}")
    # two rectangles that tile the frame, the second call into the first one's buffers
    a = run(ctx, p, lens, 5, (0, 0, 10, 16))
    b = run(ctx, p, lens, 5, (10, 0, 14, 16), into=a[:2])
    assert_bits(b[0], whole[0], "two rectangles: sum")
    assert_bits(b[1], whole[1], "two rectangles: rgb")
    for k in R.COUNTERS:
        assert a[2][k] + b[2][k] == whole[2][k]


@pytest.mark.parametrize("trav", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE], ids=["fast", "reference"])
def test_block_loop_and_rounds(trav, monkeypatch):
    """A 40 x 24 frame: 15 tiles, 960 slots x 3 chunks.  ZRT_RADIANCE_GRID=2: six trips of the
    block loop; ZRT_RADIANCE_PARTIAL_CAP = one chunk of every slot: three rounds."""
    name, model = "wraps", "thin"
    fr = ref_most(name, model, 1, 12, w=40, h=24, most=9)
    ctx, lens, p = ctx_of(name), lens_of(name, model), cparams(1, 12, trav, w=40, h=24)
    plain = run(ctx, p, lens, 9)
    check(plain, fr, "40 x 24")
    assert ctx.debug_radiance()["grid"] == 12  # ceil(960 * 3 / 256)
    monkeypatch.setenv("ZRT_RADIANCE_GRID", "2")
    check(run(ctx, p, lens, 9), fr, "two blocks")
    assert ctx.debug_radiance()["grid"] == 2
    rect = (5, 3, 30, 19)  # 4 x 3 tiles, 768 slots, ragged on both sides
    check(run(ctx, p, lens, 9, rect), sub(fr, rect), "two blocks, a ragged rectangle")
    monkeypatch.delenv("ZRT_RADIANCE_GRID")
    cap = 960 * 16
    assert z.debug_camera_plan(p, z.camera_query(0, 0, 40, 24, 9), 256, cap)["radiance"]["rounds"] == 3
    monkeypatch.setenv("ZRT_RADIANCE_PARTIAL_CAP", str(cap))
    check(run(ctx, p, lens, 9), fr, "three rounds")
    assert ctx.debug_radiance()["grid"] == 4  # a round of one chunk: 960 items
    monkeypatch.setenv("ZRT_RADIANCE_PARTIAL_CAP", str(2 * cap))  # two rounds: 2 chunks, then 1
    check(run(ctx, p, lens, 9), fr, "two rounds")


# ---- 4. accumulation -----------------------------------------------------------------------

def test_accumulation():
    """[0, 8) + [8, 16) and [0, 4) + [4, 16) at chunk 4 equal one call over [0, 16)."""
    name, model = "glass-inside", "thin"
    fr = ref_most(name, model, 0, 6, most=16)
    ctx, lens, p = ctx_of(name), lens_of(name, model), cparams(0, 6)
    whole = run(ctx, p, lens, 16)
    check(whole, fr, "one call")
    for cut in (8, 4):
        first = run(ctx, p, lens, cut)
        check(first, fr.prefix(cut), f"[0, {cut})")
        second = run(ctx, p, lens, 16 - cut, first_sample=cut, into=first[:2], accumulate=True)
        assert_bits(second[0], whole[0], f"[0, {cut}) + [{cut}, 16): sum")
        assert_bits(second[1], whole[1], f"[0, {cut}) + [{cut}, 16): rgb")
        assert second[2]["samples"] == W * H * (16 - cut)
    # without the flag a later range stands alone: its own sum and its own mean
    alone = run(ctx, p, lens, 8, first_sample=8)
    want = R.chunk_sums(fr.cols[:, 8:], CHUNK)
    assert_bits(alone[0][fr.R], want, "samples [8, 16) alone")
    assert_bits(alone[1][fr.R], R.mean_of(want, 8), "their mean")
    with pytest.raises(z.ZrtError) as e:
        run(ctx, p, lens, 10, first_sample=6, into=whole[:2], accumulate=True)
    assert e.value.code == _ffi.ZRT_E_INVALID


# ---- 5. the device error convention --------------------------------------------------------

@pytest.mark.parametrize("trav", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY], ids=["fast", "binary"])
def test_stack_overflow_is_reported(scenes, trav, monkeypatch):
    """A stack too small for the bunny's tree (ZRT_DEBUG_STACK_CAP, as
    test_radiance_stack_overflow_is_reported uses it): NaN in the rectangle only,
    ZRT_E_UNSUPPORTED once, then a correct answer (the pinhole: oracle_render's frame)."""
    s = scenes(2)
    p = cparams(0, 6, trav, w=16, h=16, spp=2)
    lens = CR.lens_of_camera(s.camera)
    rect = (3, 5, 13, 9)
    _, _, Rs = CR.pixels_of(16, rect)
    ctx = z.RenderContext(s, p)
    try:
        monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
        got = run(ctx, p, lens, 2, rect, sync=False)
        with pytest.raises(z.ZrtError) as e:
            ctx.sync()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and "overflow" in str(e.value)
        assert np.isnan(got[0][Rs, :3]).all() and (got[0][Rs, 3] == 0).all() and np.isnan(got[1][Rs]).all()
        rest = np.ones(256, bool)
        rest[Rs] = False
        assert (got[0][rest] == F(FILL)).all() and (got[1][rest] == F(FILL)).all()
        ctx.sync()  # reported once
        monkeypatch.delenv("ZRT_DEBUG_STACK_CAP")
        want, _ = O.render(s.view, s.camera, p)
        after = run(ctx, p, lens, 2, rect)
        assert_bits(after[1][Rs], want.reshape(-1, 3)[Rs], "after the error")
        assert (after[1][rest] == F(FILL)).all()
    finally:
        ctx.close()


# ---- 6. no interference --------------------------------------------------------------------

def test_a_call_leaves_runs_and_streams_alone():
    import torch
    name = "wraps"
    view, cam = S.get(name)[1], S.get(name)[2]
    p = z.RenderParams(32, 32, 8, 6, sample_chunk=2)
    fr = ref_most(name, "fisheye", 0, 12, most=5)
    pq, lens = cparams(0, 12), lens_of(name, "fisheye")

    def run_pass(with_query):
        ctx = z.RenderContext(view, p)
        try:
            tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
            frame = torch.zeros(32 * 32 * 3, dtype=torch.float32, device="cuda")
            ctx.accum_begin(cam, p)
            ctx.accum_pass(4, tiles.data_ptr())
            if with_query:
                check(run(ctx, pq, lens, 5), fr, "between two passes")
                stream = torch.cuda.Stream()
                check(run(ctx, pq, lens, 5, stream=stream.cuda_stream), fr, "on a torch stream")
            ctx.accum_pass(4, tiles.data_ptr())
            ctx.assemble(p, tiles.data_ptr(), frame.data_ptr())
            ctx.sync()
            torch.cuda.synchronize()
            out = frame.cpu().numpy().reshape(32, 32, 3).copy(), ctx.stats(), ctx.accum_info()
            if with_query:
                check(run(ctx, pq, lens, 5), fr, "after the run")
                assert all(ctx.stats()[k] == out[1][k] for k in STAT_KEYS), "a query changed zrt_ctx_stats"
            return out
        finally:
            ctx.close()

    plain, st0, info0 = run_pass(False)
    mixed, st1, info1 = run_pass(True)
    assert np.array_equal(plain.view(np.uint32), mixed.view(np.uint32))
    for k in STAT_KEYS:
        assert st0[k] == st1[k], k
    assert {k: v for k, v in info0.items() if not k.endswith("_ms")} == {k: v for k, v in info1.items()
                                                                          if not k.endswith("_ms")}
    want, _ = O.render(view, cam, p)
    assert np.array_equal(plain.view(np.uint32), want.view(np.uint32))


# ---- 7. refusals on a context --------------------------------------------------------------

def test_refusals_on_a_context():
    import torch
    ctx, p, lens = ctx_of("wraps"), cparams(), lens_of("wraps", "thin")
    s = torch.zeros((W * H + 1, 4), dtype=torch.float32, device="cuda")
    c = torch.zeros(W * H * 3 + 1, dtype=torch.float32, device="cuda")
    q = z.camera_query(0, 0, W, H, 4)

    def refused(*a):
        with pytest.raises(z.ZrtError) as e:
            ctx.camera(*a)
        assert e.value.code == _ffi.ZRT_E_INVALID

    refused(p, lens, q, 0)
    refused(p, lens, q, s.data_ptr() + 4)
    refused(p, lens, q, s.data_ptr(), c.data_ptr() + 2)
    refused(p, lens, z.camera_query(0, 0, W + 1, H, 4), s.data_ptr())
    refused(p, lens, z.camera_query(0, 0, 0, H, 4), s.data_ptr())
    refused(p, lens, z.camera_query(0, 0, W, H, 0), s.data_ptr())
    refused(p, lens, z.camera_query(0, 0, W, H, 4, flags=2), s.data_ptr())
    refused(p, lens, z.camera_query(0, 0, W, H, 4, 2, z.ZRT_CQ_ACCUMULATE), s.data_ptr())
    refused(cparams(bvh=False), lens, q, s.data_ptr())  # params that do not fit the context
    refused(cparams(trav=9), lens, q, s.data_ptr())
    bad = z.lens_init(z.ZRT_LENS_THIN, *POSES["wraps"])
    bad.kind = 5
    refused(p, bad, q, s.data_ptr())
    bad = z.lens_init(z.ZRT_LENS_THIN, *POSES["wraps"])
    bad.axis_u.y = float("nan")
    refused(p, bad, q, s.data_ptr())
    bad = z.lens_init(z.ZRT_LENS_FISHEYE, *POSES["wraps"])
    bad.half_fov = 0.0
    refused(p, bad, q, s.data_ptr())
    torch.cuda.synchronize()
    assert not s.cpu().numpy().any() and not c.cpu().numpy().any(), "a refused call wrote"
    # a 16-byte aligned dev_sum and a 4-byte aligned dev_rgb inside buffers are served
    ctx.camera(p, lens, q, s.data_ptr() + 16, c.data_ptr() + 4)
    ctx.sync()
    torch.cuda.synchronize()
    want = run(ctx, p, lens, 4)
    assert_bits(s.cpu().numpy()[1:], want[0], "a dev_sum inside a buffer")
    assert_bits(c.cpu().numpy()[1:].reshape(-1, 3), want[1], "a dev_rgb inside a buffer")
    assert not s.cpu().numpy()[0].any() and c.cpu().numpy()[0] == 0


# ---- 8. the one-shot call, the wrappers and the CLI ----------------------------------------

def test_one_shot_and_wrappers():
    name, model = "wraps", "fisheye"
    view = S.get(name)[1]
    fr = ref_most(name, model, 0, 12, most=5)
    lens = lens_of(name, model)
    for trav in TRAVERSALS:
        sums = np.zeros((H, W, 4), F)
        rgb, info = z.render_lens(view, cparams(0, 12, trav), lens, 5, sum=sums)
        assert_bits(rgb.reshape(-1, 3)[fr.R], fr.rgb, f"one-shot, traversal {trav}")
        assert_bits(sums.reshape(-1, 4)[fr.R], fr.sum, "one-shot: sums")
        assert_info(info, fr.info, "one-shot")
    # a rectangle: the frame the caller holds stays outside it; accumulation through the wrapper
    p = cparams(0, 12)
    rect = (3, 5, 13, 9)
    part = sub(fr, rect)
    sums, rgb = np.full((H, W, 4), FILL, F), np.full((H, W, 3), FILL, F)
    _, info = z.render_lens(view, p, lens, 4, rect=rect, sum=sums, rgb=rgb)
    assert info["samples"] == 13 * 9 * 4
    _, info = z.render_lens(view, p, lens, 1, rect=rect, first_sample=4, sum=sums, rgb=rgb)
    assert info["samples"] == 13 * 9
    check((sums.reshape(-1, 4), rgb.reshape(-1, 3), {**part.info, "kernel_ms": 1.0}), part, "one-shot rectangle, [0, 4) + [4, 5)")
    rgb, _ = z.render_lens(view, cparams(0, 12, bvh=False), lens_of(name, "pinhole"), 5)
    assert_bits(rgb.reshape(-1, 3), ref(name, "pinhole", 0, 5, 12, bvh=False).rgb, "one-shot, surface list")
    with pytest.raises(z.ZrtError) as e:
        z.render_lens(view, p, lens, 0)
    assert e.value.code == _ffi.ZRT_E_INVALID


CLI_DROP = ("ZRT_PASS_SAMPLES", "ZRT_DEVICES", "ZRT_ADAPTIVE_TOL", "ZRT_DENOISE", "ZRT_TEMPORAL_FRAMES",
            "ZRT_AO_SAMPLES", "ZRT_AO_RADIUS", "ZRT_AO_OUT", "ZRT_PANORAMA_OUT", "ZRT_PANORAMA_WIDTH", "ZRT_SAMPLE_CHUNK",
            "ZRT_LENS", "ZRT_LENS_OUT", "ZRT_APERTURE", "ZRT_FOCUS_DIST", "ZRT_FISHEYE_FOV")
# model, kind, the CLI's variables, the same as lens_from_camera's arguments (aperture, focus_dist, fisheye_fov)
CLI_LENSES = [("fisheye", z.ZRT_LENS_FISHEYE, {"ZRT_FISHEYE_FOV": "150"}, (0.0, 0.0, 150.0)),
              ("thin", z.ZRT_LENS_THIN, {"ZRT_APERTURE": "0.25", "ZRT_FOCUS_DIST": "2.5"}, (0.25, 2.5, 180.0)),
              ("ortho", z.ZRT_LENS_ORTHO, {"ZRT_FOCUS_DIST": "3"}, (0.0, 3.0, 180.0)),
              ("equirect", z.ZRT_LENS_EQUIRECT, {}, (0.0, 0.0, 180.0)),
              ("pinhole", z.ZRT_LENS_PINHOLE, {}, (0.0, 0.0, 180.0))]


def lens_from_restatement(kind, cam, aperture, focus, fov):
    """The lens the CLI must build, from tests/camera_ref.py's numpy restatement (not from the library)."""
    want = CR.lens_from_camera_np(kind, cam, aperture, focus, fov)
    v3 = lambda a: _ffi.Vec3(*[float(x) for x in a])
    return _ffi.Lens(kind=kind, half_fov=float(want["half_fov"]),
                     **{k: v3(want[k]) for k in ("origin", "lower_left_corner", "horizontal", "vertical", "axis_u",
                                                 "axis_v", "axis_w")})


def cli_frame(scene_index, size, samples, depth, tmp_path, env, name, extra):
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    args = [exe, str(size), str(size), str(samples), str(depth), str(scene_index)]
    r = subprocess.run(args + [str(tmp_path / "plain.png")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Lens frame" not in r.stderr
    e2 = {**env, **extra, "ZRT_LENS": name, "ZRT_LENS_OUT": str(tmp_path / f"{name}.png")}
    r = subprocess.run(args + [str(tmp_path / "out.png")], env=e2, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"  Lens frame:            {name}, {size}x{size}, {samples} samples per pixel" in r.stderr
    assert (tmp_path / "out.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    return r.stderr, (tmp_path / f"{name}.png").read_bytes()


@pytest.mark.parametrize("name,kind,extra,args", CLI_LENSES, ids=[c[0] for c in CLI_LENSES])
def test_cli_lens_frame(scenes, tmp_path, name, kind, extra, args):
    """zrt-raytrace 32 32 2 5 1 out.png with ZRT_LENS / ZRT_LENS_OUT on scene 1 (three balls, cheap
    for the oracle): the frame beside it is the one written without them, and the lens frame is the
    PNG of the reference frame (tests/camera_ref.py) of the lens restated in numpy from the scene's
    camera: 2048 one-sample oracle renders, quantised by the same writer."""
    s = scenes(1)
    env = {k: v for k, v in os.environ.items() if k not in CLI_DROP}
    err, png = cli_frame(1, 32, 2, 5, tmp_path, env, name, extra)
    p = z.RenderParams(32, 32, 2, 5)
    fr = CR.Frame(O, s.view, p, lens_from_restatement(kind, s.camera, *args), 2)
    assert f"{fr.info['rays']} rays" in err
    img = fr.image(fr.rgb)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 64  # (a picture, not a flat plane)
    z.write_png(str(tmp_path / "want.png"), np.ascontiguousarray(img))
    assert png == (tmp_path / "want.png").read_bytes()
    if name == "pinhole":  # the scene camera's own frame: the oracle's, quantised
        want, _ = O.render(s.view, s.camera, p)
        z.write_png(str(tmp_path / "oracle.png"), want)
        assert png == (tmp_path / "oracle.png").read_bytes()


def test_cli_lens_frame_on_the_bunny(scenes, tmp_path):
    """The same through the BVH: the bunny's 8 x 8 fisheye frame of one sample against the reference
    frame (64 oracle renders of a 5 k-triangle scene)."""
    s = scenes(2)
    env = {k: v for k, v in os.environ.items() if k not in CLI_DROP}
    err, png = cli_frame(2, 8, 1, 5, tmp_path, env, "fisheye", {"ZRT_FISHEYE_FOV": "100"})
    fr = CR.Frame(O, s.view, z.RenderParams(8, 8, 1, 5), lens_from_restatement(z.ZRT_LENS_FISHEYE, s.camera, 0.0, 0.0, 100.0), 1)
    assert f"{fr.info['rays']} rays" in err and fr.info["reflections"] > 8, "the frame misses the scene"
    z.write_png(str(tmp_path / "want.png"), np.ascontiguousarray(fr.image(fr.rgb)))
    assert png == (tmp_path / "want.png").read_bytes()


def test_cli_lens_refusals(tmp_path):
    """A lens option without ZRT_LENS and ZRT_LENS_OUT, an unknown model or a malformed number: refused
    before anything is rendered."""
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    env = {k: v for k, v in os.environ.items() if k not in CLI_DROP}
    for bad in ({"ZRT_LENS": "telephoto", "ZRT_LENS_OUT": "x.png"}, {"ZRT_LENS": "thin"}, {"ZRT_LENS_OUT": "x.png"},
                {"ZRT_APERTURE": "0.1"}, {"ZRT_LENS": "thin", "ZRT_LENS_OUT": "x.png", "ZRT_APERTURE": "wide"},
                {"ZRT_LENS": "fisheye", "ZRT_LENS_OUT": "x.png", "ZRT_FISHEYE_FOV": "0"}):
        r = subprocess.run([exe, "32", "32", "2", "5", "1", str(tmp_path / "out.png")], env={**env, **bad},
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "lens frame" in r.stderr
        assert not (tmp_path / "out.png").exists()

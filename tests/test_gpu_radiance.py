"""GPU tests of the radiance queries (zrt.h "radiance queries"): rayColor along
caller-supplied rays on a resident context, bit for bit against tests/radiance_ref.py
(the oracle's own pixel, composed from oracle_render alone).

1. sums, means and counters equal the reference on every traversal and on the surface
   list, both PRNGs, at wave and block edges of the ray count, over whole, ragged and
   single chunks, at depths 0, 1, 2 and 12 (past the plan's LDS attenuation rows);
2. the bunny's deep tree; 3. a block loop of several trips and a call of several rounds;
4. accumulation over sample ranges; 5. first_ray and split batches; 6. degenerate rays;
7. the device error convention; 8. no interference with runs, renders and streams;
9. the one-shot call, the Python wrapper and the CLI's panorama.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

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
COUNTS = (1, 63, 64, 65, 257)  # a lane, a wave's edges, past a block
CHUNK = 4
# (samples, max_depth) at sample_chunk 4: one sample, a ragged chunk, a whole chunk, one and two
# chunks and a ragged one; depth 0 (no ray), 1 (no row), 2, and 12 (rows 0 .. 10, past the LDS rows)
CASES = [(1, 0), (3, 1), (4, 2), (5, 12), (9, 12)]
FILL = -7.5  # what over-allocated outputs hold past n
N_RAYS = 257
STAT_KEYS = ("rays_processed", "reflections", "background_hits", "recursion_depth_hits", "samples_processed",
             "pixels_processed")


def rparams(prng=0, depth=6, trav=z.ZRT_TRAVERSAL_FAST, bvh=True, chunk=CHUNK, seed=42):
    return z.RenderParams(1, 1, 1, depth, bounded_volume_hierarchy=bvh, seed=seed, prng=prng, traversal=trav,
                          sample_chunk=chunk)


def rays_of(o, d):
    return np.ascontiguousarray(np.concatenate([np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)], 1))


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ctx, p, rays_dev, n, n_samples, first_sample=0, first_ray=0, sum0=None, stream=0, sync=True, rgb=True):
    """One zrt_ctx_radiance call over the first n rays: (sum float32[n, 4], rgb float32[n, 3] or
    None, info).  The outputs are 16 rays longer and keep their fill there."""
    import torch
    s = torch.full((n + 16, 4), FILL, dtype=torch.float32, device="cuda")
    if sum0 is not None:
        s[:n] = to_dev(np.ascontiguousarray(sum0, F))
    c = torch.full((n + 16, 3), FILL, dtype=torch.float32, device="cuda") if rgb else None
    torch.cuda.synchronize()  # (the fills ran on torch's current stream)
    rq = z.radiance_settings(n_samples, first_sample, first_ray, z.ZRT_RQ_ACCUMULATE if sum0 is not None else 0)
    ctx.radiance(p, rq, rays_dev.data_ptr(), n, s.data_ptr(), c.data_ptr() if rgb else 0, stream)
    if sync:
        ctx.sync()
    torch.cuda.synchronize()
    sh = s.cpu().numpy()
    assert (sh[n:] == F(FILL)).all(), "a query wrote sums past n"
    ch = None
    if rgb:
        ch = c.cpu().numpy()
        assert (ch[n:] == F(FILL)).all(), "a query wrote colours past n"
        ch = ch[:n]
    return sh[:n], ch, (ctx.radiance_info() if sync else None)


def assert_bits(got, want, what):
    bad = ~R.same_bits(got, want)
    assert not bad.any(), (f"{what}: {int(bad.any(-1).sum())} of {len(got)} rays differ, first "
                           f"{int(np.argmax(bad.any(-1)))}: {got[np.argmax(bad.any(-1))]} != {want[np.argmax(bad.any(-1))]}")


def assert_info(info, want, what):
    for k in R.COUNTERS:
        assert info[k] == want[k], f"{what}: {k} {info[k]} != {want[k]}"
    assert info["rays"] == info["samples"] + info["reflections"] - info["recursion_depth_hits"]
    assert info["kernel_ms"] > 0


# ---- the cases: scenes, rays and references, built once ----------------------------------

@functools.lru_cache(maxsize=None)
def shading_rays():
    return R.scattered_rays(N_RAYS, seed=11)


class Ref:
    """The reference of one (view, rays, params, samples): sums, means and per-ray counters
    of the whole batch; a call over the first n rays is their prefix."""

    def __init__(self, view, o, t, p, n_samples, first_ray=0, sums=True):
        self.rgb, self.counters = R.expected_per_ray(O, view, p, o, t, n_samples, first_ray)
        if sums:
            self.sum = R.chunk_sums(R.sample_colors(O, view, p, o, t, 0, n_samples, first_ray), p.sample_chunk)
            assert R.same_bits(R.mean_of(self.sum, n_samples), self.rgb).all()
        else:  # two samples: the mean is the sum halved, exactly
            assert n_samples == 2
            self.sum = np.zeros((len(self.rgb), 4), F)
            self.sum[:, :3] = self.rgb * F(2.0)

    def check(self, got, n, what):
        s, c, info = got
        assert_bits(s, self.sum[:n], what + ": sum")
        assert_bits(c, self.rgb[:n], what + ": rgb")
        assert_info(info, R.info_of(self.counters[:n]), what)


@functools.lru_cache(maxsize=None)
def shading_ref(name, prng, n_samples, depth, bvh=True):
    o, t = shading_rays()
    return Ref(S.get(name)[1], o, t, rparams(prng, depth, bvh=bvh), n_samples)


_CTX = {}


def shading_ctx(name, bvh=True):
    """(context, the rays on the device), kept for the session."""
    if (name, bvh) not in _CTX:
        o, t = shading_rays()
        _CTX[name, bvh] = (z.RenderContext(S.get(name)[1], rparams(bvh=bvh)), to_dev(rays_of(o, R.directions(o, t))))
    return _CTX[name, bvh]


def camera_rays(cam, w, h):
    """The pixel-centre rays of a w x h frame as (origins, targets on the view plane)."""
    o, d = S.primary_rays(cam, w, h)
    t = (o + d).astype(F)
    t[t == 0] = F(0.0)
    return o, t


# ---- 1. equals the reference ---------------------------------------------------------------

@pytest.mark.parametrize("name", S.NAMES)
@pytest.mark.parametrize("prng", PRNGS, ids=PRNG_IDS)
@pytest.mark.parametrize("n_samples,depth", CASES)
def test_radiance_equals_the_reference(name, prng, n_samples, depth):
    ref = shading_ref(name, prng, n_samples, depth)
    ctx, rays = shading_ctx(name)
    for trav in TRAVERSALS:
        p = rparams(prng, depth, trav)
        for n in COUNTS:
            ref.check(run(ctx, p, rays, n, n_samples), n, f"{name}, traversal {trav}, n {n}")
        dbg = ctx.debug_radiance()
        print(f"{name} traversal {trav} depth {depth}: {dbg}")
        if depth == 12:
            # a path the reference ended at the depth limit pushed rows 0 .. 10: past the plan's LDS rows
            assert dbg["att_lds_rows"] < depth - 1, "the plan holds every attenuation row in LDS"
            ended = R.info_of(ref.counters)["recursion_depth_hits"]
            assert ended > 0 or name not in ("glass-inside", "poles"), "no path of the reference reaches the depth limit"
            if ended:
                assert dbg["deepest_path_rows"] == depth - 1 > dbg["att_lds_rows"]


@pytest.mark.parametrize("name", ["bubbles", "wraps"])
@pytest.mark.parametrize("prng", PRNGS, ids=PRNG_IDS)
@pytest.mark.parametrize("n_samples,depth", [(4, 2), (5, 12)])
def test_radiance_on_the_surface_list(name, prng, n_samples, depth):
    """bounded_volume_hierarchy = 0: the list in the reference's order, whatever the traversal."""
    ref = shading_ref(name, prng, n_samples, depth, bvh=False)
    ctx, rays = shading_ctx(name, bvh=False)
    for trav in (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE):
        for n in COUNTS:
            ref.check(run(ctx, rparams(prng, depth, trav, bvh=False), rays, n, n_samples), n, f"{name}, list, n {n}")


@pytest.mark.parametrize("prng", PRNGS, ids=PRNG_IDS)
def test_radiance_on_a_scene_without_a_bvh(scenes, prng):
    """Scene 1 has fewer than 11 surfaces: the list although the flag asks for a BVH."""
    s = scenes(1)
    o, t = camera_rays(s.camera, 13, 5)
    p = rparams(prng, 8)
    ref = Ref(s.view, o, t, p, 5)
    assert (ref.rgb != ref.rgb[0]).any()
    ctx = z.RenderContext(s, p)
    try:
        rays = to_dev(rays_of(o, R.directions(o, t)))
        for n in (1, 64, 65):
            ref.check(run(ctx, p, rays, n, 5), n, f"scene 1, n {n}")
    finally:
        ctx.close()


# ---- 2. a deep tree ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bunny_rays():
    """128 rays at scene 2: 64 pixel centres of an 8 x 8 frame, 64 from scattered origins at the bunny."""
    cam = z.load_scene(2).camera
    o1, t1 = camera_rays(cam, 8, 8)
    o2, t2 = R.scattered_rays(64, seed=3, centre=(-0.017, 0.11, 0.0), radius=0.4, spread=0.05)
    return np.concatenate([o1, o2]), np.concatenate([t1, t2])


_BUNNY = {}


def bunny_ref(scenes, depth=6):
    if depth not in _BUNNY:
        o, t = bunny_rays()
        _BUNNY[depth] = Ref(scenes(2).view, o, t, rparams(0, depth), 2, sums=False)
    return _BUNNY[depth]


def test_radiance_on_the_bunny(scenes):
    s = scenes(2)
    ref = bunny_ref(scenes)
    hits = R.info_of(ref.counters)
    assert hits["reflections"] > 64, "the rays miss the bunny"
    o, t = bunny_rays()
    ctx = z.RenderContext(s, rparams())
    try:
        rays = to_dev(rays_of(o, R.directions(o, t)))
        for trav in (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY):
            ref.check(run(ctx, rparams(0, 6, trav), rays, 128, 2), 128, f"bunny, traversal {trav}")
    finally:
        ctx.close()


# ---- 3. the block loop and the rounds ------------------------------------------------------

@pytest.mark.parametrize("trav", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY], ids=["fast", "binary"])
def test_radiance_block_loop_of_several_trips(trav, monkeypatch):
    """ZRT_RADIANCE_GRID=2 on 257 rays x 3 chunks: 771 items on 512 lanes."""
    ref = shading_ref("bubbles", 0, 9, 12)
    ctx, rays = shading_ctx("bubbles")
    p = rparams(0, 12, trav)
    plain = run(ctx, p, rays, N_RAYS, 9)
    assert ctx.debug_radiance()["grid"] == 4
    monkeypatch.setenv("ZRT_RADIANCE_GRID", "2")
    looped = run(ctx, p, rays, N_RAYS, 9)
    assert ctx.debug_radiance()["grid"] == 2
    monkeypatch.delenv("ZRT_RADIANCE_GRID")
    assert_bits(looped[0], plain[0], "sum")
    assert_bits(looped[1], plain[1], "rgb")
    ref.check(looped, N_RAYS, "two blocks")
    monkeypatch.setenv("ZRT_RADIANCE_GRID", "1")
    ref.check(run(ctx, p, rays, 65, 9), 65, "one block, 65 rays")


@pytest.mark.parametrize("trav", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE], ids=["fast", "reference"])
def test_radiance_call_of_several_rounds(trav, monkeypatch):
    """ZRT_RADIANCE_PARTIAL_CAP = one chunk of every ray: 3 rounds for 9 samples at chunk 4."""
    ref = shading_ref("wraps", 1, 9, 12)
    ctx, rays = shading_ctx("wraps")
    p = rparams(1, 12, trav)
    plain = run(ctx, p, rays, N_RAYS, 9)
    cap = N_RAYS * 16
    assert z.debug_radiance_plan(p, z.radiance_settings(9), N_RAYS, 256, cap)["rounds"] == 3
    monkeypatch.setenv("ZRT_RADIANCE_PARTIAL_CAP", str(cap))
    rounds = run(ctx, p, rays, N_RAYS, 9)
    assert ctx.debug_radiance()["grid"] == 2  # a round of one chunk: 257 items
    assert_bits(rounds[0], plain[0], "sum")
    assert_bits(rounds[1], plain[1], "rgb")
    ref.check(rounds, N_RAYS, "three rounds")
    monkeypatch.setenv("ZRT_RADIANCE_PARTIAL_CAP", str(2 * cap))  # two rounds: 2 chunks, then 1
    ref.check(run(ctx, p, rays, N_RAYS, 9), N_RAYS, "two rounds")


def test_radiance_chunk_past_the_sample_field():
    """A sample_chunk of 2^31 or 2^32 - 1 is one sequential sum, as any chunk >= n_samples."""
    ctx, rays = shading_ctx("bubbles")
    want = run(ctx, rparams(0, 6, chunk=16), rays, 65, 9)
    for chunk in (1 << 31, (1 << 32) - 1, 65536, 65537):
        got = run(ctx, rparams(0, 6, chunk=chunk), rays, 65, 9)
        assert_bits(got[0], want[0], f"chunk {chunk}: sum")
        assert_bits(got[1], want[1], f"chunk {chunk}: rgb")


# ---- 4. accumulation -----------------------------------------------------------------------

@pytest.mark.parametrize("chunk", [4, 8])
def test_radiance_accumulates(chunk):
    """[0, 8) + [8, 16) (and, at chunk 4, [0, 4) + [4, 16)) equal one call over [0, 16): sums and means."""
    name, n = "bubbles", 65
    o, t = shading_rays()
    ctx, rays = shading_ctx(name)
    p = rparams(0, 6, chunk=chunk)
    whole = run(ctx, p, rays, n, 16)
    want = R.chunk_sums(R.sample_colors(O, S.get(name)[1], p, o[:n], t[:n], 0, 16), chunk)
    assert_bits(whole[0], want, "one call against the reference")
    assert_bits(whole[1], R.mean_of(want, 16), "one call's mean")
    for cut in (8, 4) if chunk == 4 else (8,):
        first = run(ctx, p, rays, n, cut)
        second = run(ctx, p, rays, n, 16 - cut, first_sample=cut, sum0=first[0])
        assert_bits(second[0], whole[0], f"[0, {cut}) + [{cut}, 16): sum")
        assert_bits(second[1], whole[1], f"[0, {cut}) + [{cut}, 16): rgb")
        assert second[2]["samples"] == n * (16 - cut)
    # without the flag a later range stands alone: its own sum and its own mean
    alone = run(ctx, p, rays, n, 8, first_sample=8)
    cols = R.sample_colors(O, S.get(name)[1], p, o[:n], t[:n], 8, 8)
    assert_bits(alone[0], R.chunk_sums(cols, chunk), "samples [8, 16) alone")
    assert_bits(alone[1], R.mean_of(alone[0], 8), "their mean")
    if chunk == 8:
        with pytest.raises(z.ZrtError) as e:
            run(ctx, p, rays, n, 12, first_sample=4, sum0=whole[0])
        assert e.value.code == _ffi.ZRT_E_INVALID


# ---- 5. first_ray and split batches --------------------------------------------------------

@pytest.mark.parametrize("prng", PRNGS, ids=PRNG_IDS)
def test_radiance_first_ray(prng):
    first = (1 << 40) + 5
    o, t = shading_rays()
    ctx, rays = shading_ctx("wraps")
    p = rparams(prng, 6)
    ref = Ref(S.get("wraps")[1], o[:65], t[:65], p, 5, first_ray=first)
    got = run(ctx, p, rays, 65, 5, first_ray=first)
    ref.check(got, 65, "first_ray 2^40 + 5")
    assert not R.same_bits(got[1], run(ctx, p, rays, 65, 5)[1]).all(), "first_ray does not reach the stream"


def test_radiance_split_batch():
    """Two calls with first_ray offsets equal one call: ray i of the second is ray 100 + i."""
    import torch
    ctx, rays = shading_ctx("glass-inside")
    p = rparams(1, 12)
    base = 7 << 33
    whole = run(ctx, p, rays, N_RAYS, 5, first_ray=base)
    a = run(ctx, p, rays, 100, 5, first_ray=base)
    tail = rays[100:].contiguous()
    torch.cuda.synchronize()
    b = run(ctx, p, tail, N_RAYS - 100, 5, first_ray=base + 100)
    assert_bits(np.concatenate([a[0], b[0]]), whole[0], "sum")
    assert_bits(np.concatenate([a[1], b[1]]), whole[1], "rgb")
    for k in R.COUNTERS:
        assert a[2][k] + b[2][k] == whole[2][k]


# ---- 6. degenerate rays --------------------------------------------------------------------

@pytest.mark.parametrize("bvh", [True, False], ids=["bvh", "list"])
def test_radiance_degenerate_rays(bvh):
    """A zero direction, axis-parallel directions, origins far outside the scene's origin
    bound: the reference's answers, NaN where it gives NaN."""
    name = "wraps"
    view = S.get(name)[1]
    o = np.array([[0.3, 1.6, -3.4], [0.3, 1.6, -3.4], [0.2, 2.0, 0.1], [0.2, 0.5, -3.0], [-3.0, 0.4, 0.2],
                  [3.0e4, 2.0e4, -4.0e4], [0.0, 5.0e5, 0.0], [-2.0e6, 1.0, 1.0]], F)
    t = o.copy()
    t[1] += F(1.0)  # (1, 1, 1): an ordinary ray beside the zero direction of ray 0
    t[2, 1] -= F(1.0)  # straight down
    t[3, 2] += F(2.0)  # along +z
    t[4, 0] += F(0.5)  # along +x
    t[5:] = np.array([[0.1, 0.2, 0.1], [0.05, 0.3, 0.02], [0.2, 0.4, 0.3]], F)
    t[t == 0] = F(0.0)
    assert (R.directions(o, t)[0] == 0).all()
    rays = to_dev(rays_of(o, R.directions(o, t)))
    ctx, _ = shading_ctx(name, bvh)
    for prng in PRNGS:
        ref = Ref(view, o, t, rparams(prng, 6, bvh=bvh), 5)
        assert np.isnan(ref.rgb[0]).all() and np.isfinite(ref.rgb[1:]).all()
        assert (ref.counters[2:, 2] > 0).any(), "no degenerate ray hits anything"
        for trav in TRAVERSALS:
            ref.check(run(ctx, rparams(prng, 6, trav, bvh=bvh), rays, len(o), 5), len(o), f"traversal {trav}")


# ---- 7. the device error convention --------------------------------------------------------

@pytest.mark.parametrize("trav", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY], ids=["fast", "binary"])
def test_radiance_stack_overflow_is_reported(scenes, trav, monkeypatch):
    """A stack too small for the tree (ZRT_DEBUG_STACK_CAP, as test_query_stack_overflow_is_reported
    uses it): NaN in every sum.rgb and rgb, ZRT_E_UNSUPPORTED once, then a correct answer."""
    s = scenes(2)
    ref = bunny_ref(scenes)
    o, t = bunny_rays()
    ctx = z.RenderContext(s, rparams())
    try:
        rays = to_dev(rays_of(o, R.directions(o, t)))
        p = rparams(0, 6, trav)
        monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
        got = run(ctx, p, rays, 128, 2, sync=False)
        with pytest.raises(z.ZrtError) as e:
            ctx.sync()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and "overflow" in str(e.value)
        assert np.isnan(got[0][:, :3]).all() and (got[0][:, 3] == 0).all() and np.isnan(got[1]).all()
        ctx.sync()  # reported once
        monkeypatch.delenv("ZRT_DEBUG_STACK_CAP")
        ref.check(run(ctx, p, rays, 128, 2), 128, "after the error")
    finally:
        ctx.close()


# ---- 8. no interference --------------------------------------------------------------------

def test_radiance_leaves_runs_renders_and_streams_alone(scenes):
    import torch
    s = scenes(2)
    ref = bunny_ref(scenes)
    o, t = bunny_rays()
    p = z.RenderParams(32, 32, 8, 6, sample_chunk=2)
    pq = rparams(0, 6)

    def run_pass(with_query):
        ctx = z.RenderContext(s, p)
        try:
            rays = to_dev(rays_of(o, R.directions(o, t)))
            tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
            frame = torch.zeros(32 * 32 * 3, dtype=torch.float32, device="cuda")
            feat = torch.zeros(32 * 32 * 8, dtype=torch.float32, device="cuda")
            ctx.accum_begin(s.camera, p)
            ctx.accum_pass(4, tiles.data_ptr())
            if with_query:
                ref.check(run(ctx, pq, rays, 128, 2), 128, "between two passes")
            ctx.accum_pass(4, tiles.data_ptr())
            ctx.assemble(p, tiles.data_ptr(), frame.data_ptr())
            ctx.sync()
            torch.cuda.synchronize()
            img, st, info = frame.cpu().numpy().reshape(32, 32, 3).copy(), ctx.stats(), ctx.accum_info()
            ctx.features(s.camera, p, feat.data_ptr())
            if with_query:
                # beside a feature launch, on a torch stream, then a plain render that must be the oracle's
                ref.check(run(ctx, pq, rays, 128, 2), 128, "beside a feature launch")
                stream = torch.cuda.Stream()
                ref.check(run(ctx, pq, rays, 128, 2, stream=stream.cuda_stream), 128, "on a torch stream")
                assert all(ctx.stats()[k] == st[k] for k in STAT_KEYS), "a query changed zrt_ctx_stats"
                rp = z.RenderParams(16, 16, 2, 8)
                t2 = torch.zeros(ctx.tile_count(rp) * 64 * 3, dtype=torch.float32, device="cuda")
                f2 = torch.zeros(16 * 16 * 3, dtype=torch.float32, device="cuda")
                ctx.render_tiles(s.camera, rp, t2.data_ptr())
                ctx.assemble(rp, t2.data_ptr(), f2.data_ptr())
                ctx.sync()
                torch.cuda.synchronize()
                want, rst = O.render(s.view, s.camera, rp)
                assert np.array_equal(f2.cpu().numpy().reshape(16, 16, 3).view(np.uint32), want.view(np.uint32))
                assert ctx.stats()["rays_processed"] == rst["rays_processed"]
                ref.check(run(ctx, pq, rays, 128, 2), 128, "after a render")
            ctx.sync()
            torch.cuda.synchronize()
            return img, st, info, feat.cpu().numpy()
        finally:
            ctx.close()

    plain, st0, info0, feat0 = run_pass(False)
    mixed, st1, info1, feat1 = run_pass(True)
    assert np.array_equal(plain.view(np.uint32), mixed.view(np.uint32))
    assert np.array_equal(feat0.view(np.uint32), feat1.view(np.uint32))
    for k in STAT_KEYS:
        assert st0[k] == st1[k], k
    assert {k: v for k, v in info0.items() if not k.endswith("_ms")} == {k: v for k, v in info1.items()
                                                                          if not k.endswith("_ms")}
    want, _ = O.render(s.view, s.camera, p)
    assert np.array_equal(plain.view(np.uint32), want.view(np.uint32))


# ---- 9. refusals on a context --------------------------------------------------------------

def test_radiance_refusals():
    import torch
    ctx, rays = shading_ctx("wraps")
    p = rparams()
    s = torch.zeros((80, 4), dtype=torch.float32, device="cuda")
    rq = z.radiance_settings(4)

    def refused(*a, **kw):
        with pytest.raises(z.ZrtError) as e:
            ctx.radiance(*a, **kw)
        assert e.value.code == _ffi.ZRT_E_INVALID

    refused(p, rq, 0, 64, s.data_ptr())
    refused(p, rq, rays.data_ptr(), 64, 0)
    refused(p, rq, rays.data_ptr(), 64, s.data_ptr() + 4)
    refused(p, rq, rays.data_ptr() + 2, 64, s.data_ptr())
    refused(p, rq, rays.data_ptr(), 64, s.data_ptr(), s.data_ptr() + 1)
    refused(p, z.radiance_settings(0), rays.data_ptr(), 64, s.data_ptr())
    refused(p, z.radiance_settings(4, flags=4), rays.data_ptr(), 64, s.data_ptr())
    refused(p, z.radiance_settings(4, first_sample=2, flags=z.ZRT_RQ_ACCUMULATE), rays.data_ptr(), 64, s.data_ptr())
    refused(p, z.radiance_settings(4, first_ray=(1 << 48) - 63), rays.data_ptr(), 64, s.data_ptr())
    refused(rparams(bvh=False), rq, rays.data_ptr(), 64, s.data_ptr())  # params that do not fit the context
    refused(rparams(trav=9), rq, rays.data_ptr(), 64, s.data_ptr())
    ctx.radiance(p, rq, 0, 0, 0)  # n == 0: nothing is enqueued
    ctx.sync()
    # a 4-byte aligned dev_rgb inside a buffer is served
    c = torch.zeros(64 * 3 + 1, dtype=torch.float32, device="cuda")
    ctx.radiance(p, rq, rays.data_ptr(), 64, s.data_ptr(), c.data_ptr() + 4)
    ctx.sync()
    torch.cuda.synchronize()
    assert_bits(c.cpu().numpy()[1:].reshape(64, 3), run(ctx, p, rays, 64, 4)[1], "a dev_rgb inside a buffer")
    assert c.cpu().numpy()[0] == 0


# ---- 10. the one-shot call, the wrapper and the CLI ----------------------------------------

def test_one_shot_and_wrapper_equal_the_context_path():
    name = "bubbles"
    o, t = shading_rays()
    d = R.directions(o, t)
    ctx, rays = shading_ctx(name)
    view = S.get(name)[1]
    for trav in TRAVERSALS:
        p = rparams(1, 12, trav)
        want = run(ctx, p, rays, N_RAYS, 9)
        rgb, info = z.radiance(view, p, o, d, 9)
        assert_bits(rgb, want[1], f"one-shot, traversal {trav}")
        assert_info(info, want[2], "one-shot")
    shading_ref(name, 1, 9, 12).check((want[0], rgb, info), N_RAYS, "one-shot against the reference")
    # accumulation through the wrapper: [0, 4) then [4, 9)
    p = rparams(1, 12)
    sums = np.zeros((N_RAYS, 4), F)
    z.radiance(view, p, o, d, 4, sum=sums)
    rgb, info = z.radiance(view, p, o, d, 5, first_sample=4, sum=sums)
    assert_bits(sums, want[0], "accumulated sums")
    assert_bits(rgb, want[1], "accumulated mean")
    assert info["samples"] == N_RAYS * 5
    rgb, _ = z.radiance(view, rparams(0, 12, bvh=False), o[:65], d[:65], 5)
    assert_bits(rgb, shading_ref(name, 0, 5, 12, bvh=False).rgb[:65], "one-shot, surface list")
    with pytest.raises(z.ZrtError) as e:
        z.radiance(view, p, o, d, 0)
    assert e.value.code == _ffi.ZRT_E_INVALID
    rgb, info = z.radiance(view, p, o[:0], d[:0], 3)
    assert rgb.shape == (0, 3) and info["samples"] == 0


def test_cli_panorama(scenes, tmp_path):
    """zrt-raytrace 32 32 2 5 2 out.png with ZRT_PANORAMA_OUT / ZRT_PANORAMA_WIDTH=64: a 64 x 32
    panorama beside the frame, which is the one written without them; the panorama is the PNG
    of rays_equirect + radiance."""
    s = scenes(2)
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    drop = ("ZRT_PASS_SAMPLES", "ZRT_DEVICES", "ZRT_ADAPTIVE_TOL", "ZRT_DENOISE", "ZRT_TEMPORAL_FRAMES",
            "ZRT_AO_SAMPLES", "ZRT_AO_RADIUS", "ZRT_AO_OUT", "ZRT_PANORAMA_OUT", "ZRT_PANORAMA_WIDTH", "ZRT_SAMPLE_CHUNK")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    r = subprocess.run([exe, "32", "32", "2", "5", "2", str(tmp_path / "plain.png")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Panorama" not in r.stderr
    e2 = {**env, "ZRT_PANORAMA_OUT": str(tmp_path / "pano.png"), "ZRT_PANORAMA_WIDTH": "64"}
    r = subprocess.run([exe, "32", "32", "2", "5", "2", str(tmp_path / "out.png")], env=e2, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "  Panorama:              64x32, 2 samples per ray" in r.stderr
    assert (tmp_path / "out.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    cam = s.camera
    rays = z.rays_equirect((cam.origin.x, cam.origin.y, cam.origin.z), 64, 32)
    rgb, info = z.radiance(s, z.RenderParams(1, 1, 1, 5), rays[..., :3], rays[..., 3:], 2)
    assert f"{info['rays']} rays" in r.stderr
    img = rgb.reshape(32, 64, 3)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 64  # (a picture, not a flat plane)
    z.write_png(str(tmp_path / "want.png"), img)
    assert (tmp_path / "pano.png").read_bytes() == (tmp_path / "want.png").read_bytes()
    r = subprocess.run([exe, "32", "32", "2", "5", "2", str(tmp_path / "out.png")],
                       env={**e2, "ZRT_PANORAMA_WIDTH": "63"}, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "panorama" in r.stderr

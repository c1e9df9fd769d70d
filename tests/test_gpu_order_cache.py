"""The tile order kept across frames of one context.

A scheduled launch (FAST, spp >= 128) probes every tile's cost and sorts the tiles
before it renders.  The order is a cost estimate only - chunk sums land in fixed
slots - so the context keeps it under a key (camera bits, width, height, max_depth,
rank, world_size, traversal, the guard flag, the tile count) and a later frame with
the same key skips the probe and the sort: its schedule_ms is 0 and its frame is the
same, whatever its seed, sample count or generator.  ZRT_ORDER_CACHE=0 probes every
frame.

Scene 2 at 64 x 64 (64 tiles), 128 samples, depth 6.  The order itself is compared with
the stable descending sort of the probe's costs there and at 264 x 264 (1089 tiles).

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z

import test_gpu_parity as P

pytestmark = pytest.mark.gpu

BASE = z.RenderParams(64, 64, 128, 6)


def frame(ctx, scene, cam, p):
    """(frame[H, W, 3], zrt_stats, tile order) of one render of this rank's tiles on ctx,
    assembled as a world_size-1 frame (p.world_size == 1) or left as the rank's tiles."""
    import torch
    n = ctx.tile_count(p)
    tiles = torch.empty(n * 64 * 3, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ctx.render_tiles(cam, p, tiles.data_ptr(), stream)
    torch.cuda.synchronize()
    st = ctx.stats()
    order = ctx.debug_schedule()[1]
    if p.world_size != 1:
        return tiles, st, order
    out = torch.empty(p.height * p.width * 3, dtype=torch.float32, device="cuda")
    ctx.assemble(p, tiles.data_ptr(), out.data_ptr(), stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(p.height, p.width, 3), st, order


def fresh(scene, cam, p):
    """frame() on a context of its own: the probe runs."""
    ctx = z.RenderContext(scene, p)
    try:
        img, st, order = frame(ctx, scene, cam, p)
    finally:
        ctx.close()
    assert st["schedule_ms"] > 0
    return img, order


def moved(cam):
    c = type(cam).from_buffer_copy(cam)
    c.origin.x += 0.25
    return c


def costliest_first(costs):
    """The order zrt.h promises for these probe costs: descending cost, ties in tile order."""
    return np.argsort(-costs.astype(np.int64), kind="stable")


def test_second_frame_skips_the_probe(scenes, monkeypatch):
    monkeypatch.delenv("ZRT_ORDER_CACHE", raising=False)
    s = scenes(2)
    ctx = z.RenderContext(s, BASE)
    try:
        a, sa, oa = frame(ctx, s, s.camera, BASE)
        costs = ctx.debug_schedule()[0]
        b, sb, ob = frame(ctx, s, s.camera, BASE)
        c, sc, oc = frame(ctx, s, s.camera, dataclasses.replace(BASE, flags=z.ZRT_FLAG_STATS))
    finally:
        ctx.close()
    assert sa["schedule_ms"] > 0 and sa["render_ms"] > sa["schedule_ms"]
    assert sb["schedule_ms"] == 0 and sb["render_ms"] > 0
    assert sc["schedule_ms"] == 0  # (the STATS flavour of the frame: the same key)
    assert P.same_bits(a, b).all() and P.same_bits(a, c).all()
    assert sorted(oa) == list(range(64))
    np.testing.assert_array_equal(oa, ob)
    np.testing.assert_array_equal(oa, oc)
    for k in P.COUNTERS:
        assert sa[k] == sb[k] == sc[k], k
    # the order is the sort of the probe's own costs, not just some permutation
    print(f"64 tiles: {len(costs) - len(np.unique(costs))} tiles repeat another's cost")
    assert len(costs) == 64 and costs.max() > costs.min()
    np.testing.assert_array_equal(oa, costliest_first(costs))


@pytest.mark.parametrize("max_depth", [2, 20])
def test_order_is_the_stable_sort_of_the_costs(scenes, max_depth, monkeypatch):
    """Scene 2 at 264 x 264 (33 x 33 = 1089 tiles: the device sort runs more than one block),
    128 samples, no oracle: the order a scheduled launch used is the stable descending sort of
    the costs its probe recorded.  Any permutation renders the same frame, so nothing else
    notices a sort that stopped sorting.  Ties in tile order are only tested if tiles tie: the
    costs must hold a repeated value.  Seen on an MI355X: at depth 2 the probe's costs take 3
    values and every tile shares its cost with another (the largest tie 527
    tiles), so the order is stability almost alone; at depth 20 they take 6 values, 1088 tiles
    tie and one tile's cost is its own.  (The 64 tiles of test_second_frame_skips_the_probe:
    5 values, 59 tiles repeat another's.)
    """
    monkeypatch.delenv("ZRT_ORDER_CACHE", raising=False)
    s = scenes(2)
    p = z.RenderParams(264, 264, 128, max_depth)
    ctx = z.RenderContext(s, p)
    try:
        _, st, order = frame(ctx, s, s.camera, p)
        costs = ctx.debug_schedule()[0]
    finally:
        ctx.close()
    assert st["schedule_ms"] > 0
    assert len(costs) == len(order) == 1089 and sorted(order) == list(range(1089))
    values, counts = np.unique(costs, return_counts=True)
    print(f"1089 tiles: {len(values)} distinct costs, {int((counts > 1).sum())} of them repeated, "
          f"{int(counts[counts > 1].sum())} tiles in ties, the largest tie {int(counts.max())} tiles")
    assert costs.max() > costs.min()
    assert (counts > 1).any(), "no two tiles tie: the order's stability is not tested"
    np.testing.assert_array_equal(order, costliest_first(costs))


@pytest.mark.parametrize("change", [{"seed": 7}, {"samples_per_pixel": 160}, {"prng": z.ZRT_PRNG_XOSHIRO256},
                                    {"seed": 7, "samples_per_pixel": 160, "sample_chunk": 16}],
                         ids=["seed", "spp", "prng", "seed-spp-chunk"])
def test_other_samples_reuse_the_order(scenes, change, monkeypatch):
    """What the key leaves out: the frame takes the first frame's order and equals the
    frame a context of its own (which probes with these params) renders."""
    monkeypatch.delenv("ZRT_ORDER_CACHE", raising=False)
    s = scenes(2)
    p = dataclasses.replace(BASE, **change)
    ctx = z.RenderContext(s, BASE)
    try:
        _, sa, oa = frame(ctx, s, s.camera, BASE)
        b, sb, ob = frame(ctx, s, s.camera, p)
    finally:
        ctx.close()
    assert sa["schedule_ms"] > 0 and sb["schedule_ms"] == 0
    np.testing.assert_array_equal(oa, ob)
    ref, _ = fresh(s, s.camera, p)
    assert P.same_bits(b, ref).all()


def test_moved_camera_or_depth_probes_again(scenes, monkeypatch):
    monkeypatch.delenv("ZRT_ORDER_CACHE", raising=False)
    s = scenes(2)
    cam2 = moved(s.camera)
    deeper = dataclasses.replace(BASE, max_depth=7)
    smaller = dataclasses.replace(BASE, height=56)  # (another key, and fewer tiles)
    ctx = z.RenderContext(s, BASE)
    try:
        a, sa, _ = frame(ctx, s, s.camera, BASE)
        b, sb, _ = frame(ctx, s, cam2, BASE)
        b2, sb2, _ = frame(ctx, s, cam2, BASE)
        c, sc, _ = frame(ctx, s, cam2, deeper)
        d, sd, od = frame(ctx, s, cam2, smaller)
        e, se, _ = frame(ctx, s, s.camera, BASE)  # (one order is kept: the first frame's is gone)
        n_smaller = ctx.tile_count(smaller)
    finally:
        ctx.close()
    assert [x["schedule_ms"] > 0 for x in (sa, sb, sb2, sc, sd, se)] == [True, True, False, True, True, True]
    assert len(od) == n_smaller < 64
    assert P.same_bits(a, e).all() and P.same_bits(b, b2).all()
    assert not P.same_bits(a, b).all()
    assert P.same_bits(b, fresh(s, cam2, BASE)[0]).all()
    assert P.same_bits(c, fresh(s, cam2, deeper)[0]).all()
    assert P.same_bits(d, fresh(s, cam2, smaller)[0]).all()


def test_unscheduled_frames_keep_the_order(scenes, monkeypatch):
    """A frame that does not schedule (below 128 samples, or ZRT_FLAG_NO_SCHEDULE) neither
    uses nor drops the kept order."""
    monkeypatch.delenv("ZRT_ORDER_CACHE", raising=False)
    s = scenes(2)
    ctx = z.RenderContext(s, BASE)
    try:
        a, sa, oa = frame(ctx, s, s.camera, BASE)
        _, s1, o1 = frame(ctx, s, s.camera, dataclasses.replace(BASE, samples_per_pixel=8))
        _, s2, o2 = frame(ctx, s, s.camera, dataclasses.replace(BASE, flags=z.ZRT_FLAG_NO_SCHEDULE))
        b, sb, ob = frame(ctx, s, s.camera, BASE)
    finally:
        ctx.close()
    assert sa["schedule_ms"] > 0 and s1["schedule_ms"] == 0 and s2["schedule_ms"] == 0 and sb["schedule_ms"] == 0
    assert len(o1) == 0 and len(o2) == 0
    np.testing.assert_array_equal(oa, ob)
    assert P.same_bits(a, b).all()


def test_order_cache_off_always_probes(scenes, monkeypatch):
    monkeypatch.setenv("ZRT_ORDER_CACHE", "0")
    s = scenes(2)
    ctx = z.RenderContext(s, BASE)
    try:
        a, sa, oa = frame(ctx, s, s.camera, BASE)
        b, sb, ob = frame(ctx, s, s.camera, BASE)
        monkeypatch.setenv("ZRT_ORDER_CACHE", "1")
        c, sc, _ = frame(ctx, s, s.camera, BASE)  # (the last probe's order is a valid one)
    finally:
        ctx.close()
    assert sa["schedule_ms"] > 0 and sb["schedule_ms"] > 0 and sc["schedule_ms"] == 0
    np.testing.assert_array_equal(oa, ob)
    assert P.same_bits(a, b).all() and P.same_bits(a, c).all()


def test_two_ranks_have_their_own_keys(scenes, monkeypatch):
    """Ranks 0 and 1 of 2 on one context: a rank's order is not the other's (each probes
    after the other), a rank's second frame reuses its own, and the tiles are the ones
    contexts of their own render."""
    import torch
    monkeypatch.delenv("ZRT_ORDER_CACHE", raising=False)
    s = scenes(2)
    r0 = dataclasses.replace(BASE, rank=0, world_size=2)
    r1 = dataclasses.replace(BASE, rank=1, world_size=2)
    ctx = z.RenderContext(s, BASE)
    try:
        t0, s0, o0 = frame(ctx, s, s.camera, r0)
        t1, s1, o1 = frame(ctx, s, s.camera, r1)
        t1b, s1b, o1b = frame(ctx, s, s.camera, r1)
        t0b, s0b, o0b = frame(ctx, s, s.camera, r0)
        t0c, s0c, _ = frame(ctx, s, s.camera, dataclasses.replace(r0, seed=7))
    finally:
        ctx.close()
    assert [x["schedule_ms"] > 0 for x in (s0, s1, s1b, s0b, s0c)] == [True, True, False, True, False]
    assert len(o0) == 32 and len(o1) == 32
    np.testing.assert_array_equal(o1, o1b)
    np.testing.assert_array_equal(o0, o0b)
    assert torch.equal(t0.view(torch.int32), t0b.view(torch.int32))
    assert torch.equal(t1.view(torch.int32), t1b.view(torch.int32))
    for p, t in ((r0, t0), (r1, t1), (dataclasses.replace(r0, seed=7), t0c)):
        own, _ = fresh(s, s.camera, p)
        assert torch.equal(t.view(torch.int32), own.view(torch.int32)), (p.rank, p.seed)

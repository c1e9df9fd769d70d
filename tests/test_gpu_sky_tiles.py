"""The all-sky tiles' kernel against the render kernel and the oracle.

zrt_ctx_render_tiles hands the tiles the host proved all sky (tile_class.cpp) to
sky_kernel, which traces nothing, and the rest to the render kernel; ZRT_SKY_TILES=0
keeps every tile in the render kernel.  Every case renders with the split on and off,
in the timed and the STATS flavour, and asks of all four the oracle's frame bit for
bit and its Progress counters.  Scene 3's triangles leave no tile provably sky (the
split is a no-op there); scene 2 splits about 0.4 of its tiles.

Frames: 64 x 64 and 70 x 50 (ragged tiles) at 40 spp - no multiple of the chunks 7
and 32 - and 256 x 256 x 2 (1 024 tiles: past a wave, a block and a compaction round).

Run on an MI355X: ``pytest -m gpu``.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O

import test_gpu_parity as P
import test_tile_classes as TC

pytestmark = pytest.mark.gpu

XORO, XOSHI = z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256
SKY_SLOT = 47  # zrt_ctx_debug_counters: the sky tiles of the last launch
_ORACLE = {}


def lockstep(monkeypatch):
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES", "ZRT_ORDER_CACHE", "ZRT_LEAN"):
        monkeypatch.delenv(k, raising=False)


def oracle_frame(key, view, cam, p):
    k = (key, p.width, p.height, p.samples_per_pixel, p.max_depth, p.prng, p.seed, p.sample_chunk)
    if k not in _ORACLE:
        plain = z.RenderParams(p.width, p.height, p.samples_per_pixel, p.max_depth, prng=p.prng, seed=p.seed,
                               sample_chunk=p.sample_chunk)
        img, st = O.render(view, cam, plain)
        img.setflags(write=False)
        _ORACLE[k] = (img, st)
    return _ORACLE[k]


def render_ranks(scene, cam, p, world):
    """The frame assembled from `world` ranks' tiles on one context, the Progress counters
    summed over the ranks, and the sky tiles of each rank's launch."""
    import torch
    ctx = z.RenderContext(scene, p)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        parts, total, sky = [], dict.fromkeys(P.COUNTERS, 0), []
        for rank in range(world):
            pr = dataclasses.replace(p, rank=rank, world_size=world)
            buf = torch.empty(max(1, ctx.tile_count(pr)) * 64 * 3, dtype=torch.float32, device="cuda")
            ctx.render_tiles(cam, pr, buf.data_ptr(), stream)
            torch.cuda.synchronize()
            st = ctx.stats()
            for k in P.COUNTERS:
                total[k] += st[k]
            sky.append(int(ctx.debug_counters()[SKY_SLOT]))
            parts.append(buf[:ctx.tile_count(pr) * 64 * 3])
        frame = torch.empty(p.height * p.width * 3, dtype=torch.float32, device="cuda")
        ctx.assemble(dataclasses.replace(p, rank=0, world_size=world), torch.cat(parts).data_ptr(), frame.data_ptr(), stream)
        torch.cuda.synchronize()
        return frame.cpu().numpy().reshape(p.height, p.width, 3), total, sky
    finally:
        ctx.close()


def check_split(monkeypatch, key, scene, cam, p, world, want_sky):
    """Split on and off x timed and STATS against the oracle; want_sky: None (whatever the
    classifier says), or whether the split launches must have had sky tiles."""
    view = scene.view if isinstance(scene, z.LoadedScene) else scene
    ref, rs = oracle_frame(key, view, cam, p)
    n_sky = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("ZRT_SKY_TILES", knob)
        expect = [int((z.debug_tile_classes(view, cam, dataclasses.replace(p, rank=r, world_size=world))[0]
                       == z.ZRT_TILE_SKY).sum()) for r in range(world)]
        for flags in (0, z.ZRT_FLAG_STATS):
            img, total, sky = render_ranks(scene, cam, dataclasses.replace(p, flags=flags), world)
            P.assert_bit_exact(img, ref)
            for k in P.COUNTERS:
                assert total[k] == rs[k], (knob, flags, k, total[k], rs[k])
            assert sky == expect, (knob, flags, sky, expect)
        n_sky[knob] = sum(expect)
    assert n_sky["0"] == 0
    if want_sky is not None:
        assert (n_sky["1"] > 0) == want_sky, n_sky
    return n_sky["1"]


# scene, width, height, spp, depth, chunk, prng, seed, ranks
CASES = [
    (2, 64, 64, 40, 20, 7, XORO, 42, 1),
    (2, 64, 64, 40, 1, 32, XOSHI, 7, 2),
    (2, 70, 50, 40, 20, 32, XORO, 7, 3),
    (2, 70, 50, 40, 1, 7, XOSHI, 42, 1),
    (2, 256, 256, 2, 20, 32, XORO, 42, 1),
    (2, 256, 256, 2, 1, 7, XOSHI, 7, 2),
    (2, 256, 256, 2, 20, 7, XORO, 7, 3),
    (3, 64, 64, 40, 20, 7, XORO, 42, 1),
    (3, 70, 50, 40, 1, 32, XOSHI, 7, 3),
    (3, 256, 256, 2, 20, 32, XORO, 7, 2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_split_equals_oracle(scenes, case, monkeypatch):
    lockstep(monkeypatch)
    which, w, h, spp, depth, chunk, prng, seed, world = case
    s = scenes(which)
    p = z.RenderParams(w, h, spp, depth, prng=prng, seed=seed, sample_chunk=chunk)
    check_split(monkeypatch, which, s, s.camera, p, world, want_sky=(which == 2))


def test_scheduled_frame_splits_the_cost_order(scenes, monkeypatch):
    """128 spp: the probe runs, and the render kernel takes the probe's order without the
    sky tiles (compact_kernel); 40 x 40 and, past a compaction round, 264 x 264 x 128 is
    too slow for the oracle, so the larger frame is checked split on against split off."""
    lockstep(monkeypatch)
    s = scenes(2)
    p = z.RenderParams(40, 40, 128, 20, sample_chunk=32)  # (5 of its 25 tiles are sky)
    assert check_split(monkeypatch, 2, s, s.camera, p, 1, want_sky=True) > 0
    big = z.RenderParams(264, 264, 128, 2, sample_chunk=32)  # 1 089 tiles
    frames = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("ZRT_SKY_TILES", knob)
        frames[knob] = render_ranks(s, s.camera, big, 1)
    assert P.same_bits(frames["1"][0], frames["0"][0]).all()
    assert frames["1"][1] == frames["0"][1]
    assert frames["1"][2][0] > 300 and frames["0"][2] == [0]


def edge_scene(which):
    """all: twelve small spheres behind the camera, spread widely enough that the camera
    lies inside their origin bound (every tile sky).  none: the camera
    looks down at a ground sphere that fills the frame (no tile sky)."""
    if which == "all":
        prims = [("s", (1.0 * i - 5.5, 0.2, 3.0 + 0.01 * i), 0.05) for i in range(12)]
        cam = z.camera_init((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 1.0)
    else:
        prims = [("s", (0.0, -100.0, 0.0), 100.0)] + [("s", (0.4 * i - 2.0, 0.1, 0.3), 0.1) for i in range(11)]
        cam = z.camera_init((0.0, 3.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 40.0, 1.0)
    return TC.build_scene(prims), cam


@pytest.mark.parametrize("which", ["all", "none"])
def test_edge_scenes(which, monkeypatch):
    """A launch whose tiles are all sky enqueues no render kernel and still reports its
    frame, counters and status; one with no sky tile is the render kernel's alone."""
    lockstep(monkeypatch)
    s, cam = edge_scene(which)
    view = C.pointer(s)
    for p in (z.RenderParams(64, 64, 40, 20, sample_chunk=7), z.RenderParams(48, 48, 128, 20)):
        monkeypatch.setenv("ZRT_SKY_TILES", "1")
        cls, _ = z.debug_tile_classes(view, cam, p)
        assert (cls == z.ZRT_TILE_SKY).all() if which == "all" else not (cls == z.ZRT_TILE_SKY).any()
        check_split(monkeypatch, "edge-" + which, view, cam, p, 1, want_sky=(which == "all"))
        check_split(monkeypatch, "edge-" + which, view, cam, p, 2, want_sky=(which == "all"))


def test_progressive_run_takes_the_split(scenes, monkeypatch):
    """Passes of 16 of 40 samples (and of 64 of 128 on a 24 x 24 frame, scheduled: one of its nine tiles is sky): the frame of one launch,
    with the split on and off."""
    lockstep(monkeypatch)
    s = scenes(2)
    for p, step in ((z.RenderParams(40, 40, 40, 20, sample_chunk=8), 16), (z.RenderParams(24, 24, 128, 20), 64)):
        ref, rs = oracle_frame(2, s.view, s.camera, p)
        for knob in ("1", "0"):
            monkeypatch.setenv("ZRT_SKY_TILES", knob)
            img, st, infos = z.render_progressive(s, s.camera, p, step)
            assert len(infos) >= 2
            P.assert_bit_exact(img, ref)
            for k in P.COUNTERS:
                assert st[k] == rs[k], (knob, k)


def test_adaptive_run_is_unchanged(scenes, monkeypatch):
    """Adaptive levels do not take the split (their active list changes on the device):
    the same image, per-pixel samples and counters under ZRT_SKY_TILES=1 and 0."""
    lockstep(monkeypatch)
    s = scenes(2)
    p = z.RenderParams(64, 64, 256, 20)
    runs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("ZRT_SKY_TILES", knob)
        runs[knob] = z.render_adaptive(s, s.camera, p, 0.05)
    assert P.same_bits(runs["1"][0], runs["0"][0]).all()
    np.testing.assert_array_equal(runs["1"][1], runs["0"][1])
    for k in P.COUNTERS:
        assert runs["1"][2][k] == runs["0"][2][k], k


def test_order_cache_repeat_reuses_the_classes(scenes, monkeypatch):
    """The second frame with the same key probes nothing and classifies nothing: its
    schedule_ms is 0, its sky tiles and its frame are the first frame's."""
    import test_gpu_order_cache as OC
    lockstep(monkeypatch)
    monkeypatch.setenv("ZRT_SKY_TILES", "1")
    s = scenes(2)
    p = z.RenderParams(40, 40, 128, 20)
    ctx = z.RenderContext(s, p)
    try:
        a, sa, _ = OC.frame(ctx, s, s.camera, p)
        na = int(ctx.debug_counters()[SKY_SLOT])
        b, sb, _ = OC.frame(ctx, s, s.camera, dataclasses.replace(p, seed=7))
        c, sc, _ = OC.frame(ctx, s, s.camera, p)
        nc = int(ctx.debug_counters()[SKY_SLOT])
    finally:
        ctx.close()
    assert sa["schedule_ms"] > 0 and sb["schedule_ms"] == 0 and sc["schedule_ms"] == 0
    assert na > 0 and na == nc
    assert P.same_bits(a, c).all() and not P.same_bits(a, b).all()
    ref, _ = oracle_frame(2, s.view, s.camera, p)
    P.assert_bit_exact(a, ref)

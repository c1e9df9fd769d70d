"""The one-sphere tiles' kernel against the render kernel and the oracle.

zrt_ctx_render_tiles hands the tiles the host proved one-sphere (tile_class.cpp: no
camera ray of theirs can hit anything but one sphere) to render_kernel's ONE_SPHERE
instance, whose camera rays test that sphere alone instead of walking the tree;
ZRT_SPHERE_TILES=0 leaves them with the general tiles, =2 sends their list through a
launch of the unchanged render kernel.  Every case renders under the three knobs in the
timed and the STATS flavour and asks of all six the oracle's frame bit for bit and its
Progress counters; under STATS the rays are the same and the node visits fewer with the
split (a short-path ray counts one ray and one sphere test, no node).

Frames: scene 2 at 64 x 64 and 70 x 50 (ragged tiles) x 4 spp, and 64 x 64 x 128 behind the
scheduling probe (the lists in the probe's order).  The oracle needs half a minute for
each of those last frames, so its six whole frames and their Progress counters are
recorded (tests/golden/sphere_tiles_scene2_64x64x128.npz, written by
make_sphere_tiles_golden.py beside it); every run is held to the whole recorded frame and
to the counters, and the oracle renders one row of each frame again, so a record that no
longer is the oracle's fails.  The synthetic scenes of tests/sphere_scenes.py at 64 x 64 x 4,
whole frames from the oracle.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses
import os

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O

import sphere_scenes as SS
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

XORO, XOSHI = z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256
SKY_SLOT, ONE_SLOT = 47, 46  # zrt_ctx_debug_counters: the sky / one-sphere tiles of the last launch
K_RAYS, K_NODES, K_SPH = 3, 4, 6  # ... and the STATS flavour's rays, node visits, sphere tests
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sphere_tiles_scene2_64x64x128.npz")
LIVE_ROW = 31  # the row of a recorded frame the oracle renders again
_ORACLE = {}


@pytest.fixture(autouse=True)
def lockstep(monkeypatch):
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES", "ZRT_ORDER_CACHE", "ZRT_LEAN", "ZRT_SKY_TILES",
              "ZRT_SPHERE_TILES"):
        monkeypatch.delenv(k, raising=False)


def oracle_frame(key, view, cam, p, recorded=False):
    """The oracle's frame and stats, computed once; recorded: read from GOLDEN (scene 2 at
    64 x 64 x 128, chunk 32, seed 7 + depth), one row of it checked against the oracle itself."""
    k = (key, p.width, p.height, p.samples_per_pixel, p.max_depth, p.prng, p.seed, p.sample_chunk)
    if k not in _ORACLE:
        plain = z.RenderParams(p.width, p.height, p.samples_per_pixel, p.max_depth, prng=p.prng, seed=p.seed,
                               sample_chunk=p.sample_chunk)
        if recorded:
            assert (key, p.width, p.height, p.samples_per_pixel, p.sample_chunk, p.seed) == (2, 64, 64, 128, 32, 7 + p.max_depth)
            with np.load(GOLDEN) as g:
                img = g[f"frame_d{p.max_depth}_p{p.prng}"].copy()
                st = dict(zip(P.COUNTERS, (int(x) for x in g[f"counters_d{p.max_depth}_p{p.prng}"])))
            row = O.render(view, cam, plain, rows=(LIVE_ROW, LIVE_ROW + 1))[0][LIVE_ROW]
            assert P.same_bits(row, img[LIVE_ROW]).all(), "the recorded frame is not the oracle's: regenerate it"
        else:
            img, st = O.render(view, cam, plain)
        img.setflags(write=False)
        _ORACLE[k] = (img, st)
    return _ORACLE[k]


def render_ranks(scene, cam, p, world):
    """The frame assembled from `world` ranks' tiles on one context; the Progress counters,
    the STATS rays / node visits / sphere tests summed over the ranks; each rank's sky and
    one-sphere tiles."""
    import torch
    ctx = z.RenderContext(scene, p)
    stream = torch.cuda.current_stream().cuda_stream
    try:
        parts, total, sky, one, dbg = [], dict.fromkeys(P.COUNTERS, 0), [], [], np.zeros(3, np.int64)
        for rank in range(world):
            pr = dataclasses.replace(p, rank=rank, world_size=world)
            buf = torch.empty(max(1, ctx.tile_count(pr)) * 64 * 3, dtype=torch.float32, device="cuda")
            ctx.render_tiles(cam, pr, buf.data_ptr(), stream)
            torch.cuda.synchronize()
            st = ctx.stats()
            for k in P.COUNTERS:
                total[k] += st[k]
            c = ctx.debug_counters()
            sky.append(int(c[SKY_SLOT]))
            one.append(int(c[ONE_SLOT]))
            dbg += np.array([int(c[K_RAYS]), int(c[K_NODES]), int(c[K_SPH])], np.int64)
            parts.append(buf[:ctx.tile_count(pr) * 64 * 3])
        frame = torch.empty(p.height * p.width * 3, dtype=torch.float32, device="cuda")
        ctx.assemble(dataclasses.replace(p, rank=0, world_size=world), torch.cat(parts).data_ptr(), frame.data_ptr(), stream)
        torch.cuda.synchronize()
        return frame.cpu().numpy().reshape(p.height, p.width, 3), total, sky, one, dbg
    finally:
        ctx.close()


def n_one_expected(view, cam, p, world):
    out = []
    for r in range(world):
        cls, _ = z.debug_tile_classes(view, cam, dataclasses.replace(p, rank=r, world_size=world), one_sphere=True)
        out.append(int((((cls & z.ZRT_TILE_SKY) == 0) & ((cls & z.ZRT_TILE_ONE_SPHERE) != 0)).sum()))
    return out


def check_split(monkeypatch, key, scene, cam, p, recorded=False, want_one=None, all_fall_back=False):
    """ZRT_SPHERE_TILES 0, 1, 2 x timed and STATS against the oracle's whole frame and Progress
    counters (recorded: the oracle's recorded ones); then two ranks' tiles likewise.
    want_one: whether the split launches must have had one-sphere tiles (None: whatever the
    classifier says).  all_fall_back: every camera ray is degenerate, so the one-sphere
    kernel walks the tree for each.  Returns the one-sphere tiles."""
    view = scene.view if isinstance(scene, z.LoadedScene) else scene
    ref, rs = oracle_frame(key, view, cam, p, recorded)
    runs = {}
    for knob in ("0", "1", "2"):
        monkeypatch.setenv("ZRT_SPHERE_TILES", knob)
        expect = n_one_expected(view, cam, p, 1)
        for flags in (0, z.ZRT_FLAG_STATS):
            img, total, sky, one, dbg = render_ranks(scene, cam, dataclasses.replace(p, flags=flags), 1)
            print(f"{key} {p.width}x{p.height}x{p.samples_per_pixel} depth {p.max_depth} prng {p.prng} knob {knob} "
                  f"flags {flags}: sky {sky} one-sphere {one} rays/nodes/sphere tests {dbg.tolist()}")
            P.assert_bit_exact(img, ref)
            for k in P.COUNTERS:
                assert total[k] == rs[k], (knob, flags, k, total[k], rs[k])
            assert one == expect, (knob, flags, one, expect)
            runs[knob, flags] = (img, total, sky, dbg)
    base = runs["0", 0]
    for (knob, flags), (img, total, sky, dbg) in runs.items():
        assert P.same_bits(img, base[0]).all(), (knob, flags)
        assert total == base[1] and sky == base[2], (knob, flags)
    monkeypatch.setenv("ZRT_SPHERE_TILES", "1")
    n_one = n_one_expected(view, cam, p, 1)[0]
    monkeypatch.setenv("ZRT_SPHERE_TILES", "0")
    assert n_one_expected(view, cam, p, 1) == [0]
    if want_one is not None:
        assert (n_one > 0) == want_one, n_one
    S = z.ZRT_FLAG_STATS
    r0, r1, r2 = runs["0", S][3], runs["1", S][3], runs["2", S][3]
    assert r0[0] == r1[0] == r2[0] == base[1]["rays_processed"] > 0  # the rays
    assert (r0 == r2).all()  # (the unchanged kernel on another list)
    if n_one == 0 or all_fall_back:
        assert (r0 == r1).all()
    else:
        assert r1[1] < r0[1], (r0, r1)  # node visits
    # two ranks' tiles assemble to the one-rank frame
    monkeypatch.setenv("ZRT_SPHERE_TILES", "1")
    img2, total2, _, one2, _ = render_ranks(scene, cam, p, 2)
    P.assert_bit_exact(img2, ref)
    assert P.same_bits(img2, base[0]).all()
    for k in P.COUNTERS:
        assert total2[k] == rs[k], (k, total2[k], rs[k])
    assert one2 == n_one_expected(view, cam, p, 2)
    return n_one


# width, height, spp, chunk, whether the oracle's frame is the recorded one
FRAMES = [(64, 64, 4, 0, False), (70, 50, 4, 3, False), (64, 64, 128, 32, True)]


@pytest.mark.parametrize("prng", [XORO, XOSHI])
@pytest.mark.parametrize("depth", [1, 2, 20])
@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}x{f[2]}")
def test_scene_2_equals_oracle(scenes, frame, depth, prng, monkeypatch):
    w, h, spp, chunk, recorded = frame
    s = scenes(2)
    p = z.RenderParams(w, h, spp, depth, prng=prng, seed=7 + depth, sample_chunk=chunk)
    assert check_split(monkeypatch, 2, s, s.camera, p, recorded, want_one=True) >= 16


@pytest.mark.parametrize("name", ["horizon", "overlap", "behind", "inside", "two", "down_z", "slit", "all"])
def test_synthetic_scenes_equal_oracle(name, monkeypatch):
    """The horizon scene puts the sphere's silhouette - tangent rays, where the rounded
    sphere test and the loose box test can disagree - through one-sphere tiles; down_z is
    the issue's axis-parallel case (an odd width, the camera down -z): d.x == 0 there needs
    px + r - 0.5 == width / 2 exactly, which four random jitters per pixel almost never give,
    so that case by itself does not reach the ray_degenerate fallback.  slit does: every
    camera ray of it is degenerate (|d.x| < 2^-100), every lane takes traverse_wide, and the
    node visits are asked to equal the unsplit render's;
    all: a frame whose tiles are all one-sphere (the general launch is empty)."""
    _, view, cam = SS.get(name)
    for prng in (XORO, XOSHI):
        p = z.RenderParams(65 if name == "down_z" else 64, 64, 4, 20, prng=prng, seed=3)
        n = check_split(monkeypatch, name, view, cam, p, want_one=True, all_fall_back=(name == "slit"))
        if name == "all":
            assert n == 64


def test_frame_without_a_one_sphere_tile(scenes, monkeypatch):
    """Scene 3 (the teapot): no tile is provably anything; the knob changes nothing."""
    s = scenes(3)
    p = z.RenderParams(64, 64, 4, 20)
    assert check_split(monkeypatch, 3, s, s.camera, p, want_one=False) == 0


def test_progressive_run_of_three_passes(scenes, monkeypatch):
    """Three passes of 4 of 12 samples (and of 64 of 192, scheduled): the one-shot frame, under each knob."""
    s = scenes(2)
    _, hview, hcam = SS.get("horizon")
    for key, scene, view, cam, p, step in ((2, s, s.view, s.camera, z.RenderParams(40, 40, 12, 20, sample_chunk=2), 4),
                                           ("horizon", hview, hview, hcam, z.RenderParams(64, 64, 192, 20), 64)):
        ref, rs = oracle_frame(key, view, cam, p)
        for knob in ("1", "0", "2"):
            monkeypatch.setenv("ZRT_SPHERE_TILES", knob)
            img, st, infos = z.render_progressive(scene, cam, p, step)
            assert len(infos) == 3
            P.assert_bit_exact(img, ref)
            for k in P.COUNTERS:
                assert st[k] == rs[k], (knob, k)


def test_adaptive_run_is_unchanged(scenes, monkeypatch):
    """Adaptive levels do not take the split: the same image, per-pixel samples and counters
    under ZRT_SPHERE_TILES=1 and 0."""
    s = scenes(2)
    p = z.RenderParams(64, 64, 256, 20)
    runs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("ZRT_SPHERE_TILES", knob)
        runs[knob] = z.render_adaptive(s, s.camera, p, 0.05)
    assert P.same_bits(runs["1"][0], runs["0"][0]).all()
    np.testing.assert_array_equal(runs["1"][1], runs["0"][1])
    for k in P.COUNTERS:
        assert runs["1"][2][k] == runs["0"][2][k], k


def test_order_cache_repeat_reuses_the_lists(monkeypatch):
    """The second frame with the same key probes nothing and classifies nothing: its
    schedule_ms is 0, its one-sphere tiles and its frame are the first frame's."""
    import test_gpu_order_cache as OC
    monkeypatch.setenv("ZRT_SPHERE_TILES", "1")
    _, view, cam = SS.get("horizon")
    p = z.RenderParams(64, 64, 128, 20)
    ctx = z.RenderContext(view, p)
    try:
        a, sa, _ = OC.frame(ctx, view, cam, p)
        na = int(ctx.debug_counters()[ONE_SLOT])
        b, sb, _ = OC.frame(ctx, view, cam, dataclasses.replace(p, seed=7))
        c, sc, _ = OC.frame(ctx, view, cam, p)
        nc = int(ctx.debug_counters()[ONE_SLOT])
        # the STATS launch of the same frame splits alike, from the same lists
        d, sd, _ = OC.frame(ctx, view, cam, dataclasses.replace(p, flags=z.ZRT_FLAG_STATS))
        nd = int(ctx.debug_counters()[ONE_SLOT])
    finally:
        ctx.close()
    assert sa["schedule_ms"] > 0 and sb["schedule_ms"] == 0 and sc["schedule_ms"] == 0 and sd["schedule_ms"] == 0
    assert na > 0 and na == nc == nd
    assert P.same_bits(a, c).all() and P.same_bits(a, d).all() and not P.same_bits(a, b).all()
    ref, _ = oracle_frame("horizon", view, cam, p)
    P.assert_bit_exact(a, ref)

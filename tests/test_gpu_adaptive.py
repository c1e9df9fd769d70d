"""Adaptive sampling: 8x8 tiles that have converged stop being refined.

The rule (include/zrt.h, "adaptive sampling") is a deterministic f32 function of two
previews, and every preview of a run is, bit for bit, the oracle's full render at
that many samples per pixel.  expected_run() below restates the rule in numpy on the
oracle's frames at every sample level (test_gpu_loop_edges's shared frames): which
level every tile stops at, and the composite frame after every level, in which tile t
shows the oracle's frame at samples(t).  The GPU run (zrt_ctx_adapt_begin / _level /
_samples, zrt_render_adaptive, the CLI's ZRT_ADAPTIVE_TOL) is compared with that,
never with itself.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O  # noqa: F401  (the oracle behind E.oracle_frame)

import test_gpu_loop_edges as E
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = z._ffi.ZRT_E_INVALID, z._ffi.ZRT_E_UNSUPPORTED
SCANLINES = z.ZRT_FLAG_SCANLINES
TOLERANCES = [2.0 ** -k for k in range(15)]
# The oracle's frames of "wraps" at 24 x 24 have no tolerance of the grid with a mixed stop map
# at cap 24 (every tile stops before the cap, or none does), nor do "poles"'s at cap 48;
# "glass-inside" and "bubbles" have one for every case below, "wraps" for the cases at cap 48,
# behind the probe and at 20 x 12 (computed from the oracle alone, on the CPU).
SCENES = ["glass-inside", "bubbles"]


# ---- the rule, restated on the oracle's frames -------------------------------------------

def tile_boxes(p):
    """[(x0, x1, y0, y1)] of every 8x8 tile clipped to the rendered square: x and y in
    [0, height) (raytrace.zig:168's bound), tile t at column t % tiles_x, row t // tiles_x."""
    n = (p.height + 7) // 8
    return [(tx * 8, min(tx * 8 + 8, p.height), ty * 8, min(ty * 8 + 8, p.height))
            for ty in range(n) for tx in range(n)]


def tile_passes(A, H, tol):
    """zrt.h's test on the in-frame pixels of one tile, in f32, in its order; NaN compares false."""
    A, H = A.astype(np.float32), H.astype(np.float32)
    with np.errstate(invalid="ignore"):
        d = (np.abs(A[..., 0] - H[..., 0]) + np.abs(A[..., 1] - H[..., 1])) + np.abs(A[..., 2] - H[..., 2])
        s = (A[..., 0] + A[..., 1]) + A[..., 2]
        assert d.dtype == np.float32 and s.dtype == np.float32
        return bool((d <= np.float32(tol) * np.sqrt(s)).all())


@dataclasses.dataclass
class Expected:
    tol: float
    levels: list        # L_0 ..
    stop: np.ndarray    # per tile: the index of the level it stops at
    steps: list         # per level run: (tiles rendered, tiles active after)
    frames: list        # per level run: the composite frame

    def samples(self, k):
        """Samples per pixel of every tile after level k."""
        return np.array([self.levels[min(s, k)] for s in self.stop], np.uint32)


def stop_levels(frames, levels, p, tol):
    boxes = tile_boxes(p)
    last = len(levels) - 1
    stop = np.full(len(boxes), last)
    for k in range(1, last):  # decisions after every level k >= 1 but the last
        A, H = frames[levels[k]], frames[levels[k - 1]]
        for t, (x0, x1, y0, y1) in enumerate(boxes):
            if stop[t] == last and tile_passes(A[y0:y1, x0:x1], H[y0:y1, x0:x1], tol):
                stop[t] = k
    return stop


def expected_run(scenes, which, p, first, tol=None):
    """The run the rule gives on the oracle's frames.  tol None: the value of 2^-k, k = 0 .. 14,
    whose stop map has the most distinct levels (of equals the smallest, which sends most tiles
    on towards the cap)."""
    levels = z.adapt_plan(p, 0.5, first)
    frames = {L: E.oracle_frame(scenes, which, dataclasses.replace(p, samples_per_pixel=L))[0] for L in levels}
    if tol is None:
        maps = [(len(set(stop_levels(frames, levels, p, t))), i, t) for i, t in enumerate(TOLERANCES)]
        tol = max(maps)[2]
    stop = stop_levels(frames, levels, p, tol)
    boxes = tile_boxes(p)
    steps, comps = [], []
    for k in range(len(levels)):
        rendered = int((stop >= k).sum())
        if rendered == 0:
            break
        after = int((stop > k).sum())
        comp = np.zeros((p.height, p.width, 3), np.float32)
        for t, (x0, x1, y0, y1) in enumerate(boxes):
            comp[y0:y1, x0:x1] = frames[levels[min(stop[t], k)]][y0:y1, x0:x1]
        steps.append((rendered, after))
        comps.append(comp)
    return Expected(tol, levels, stop, steps, comps)


def in_frame_pixels(p):
    return np.array([(x1 - x0) * (y1 - y0) for x0, x1, y0, y1 in tile_boxes(p)], np.uint64)


def assert_mixed(ex):
    """A condition on the inputs, from the oracle alone: some tile stops early, some reaches the cap."""
    last = len(ex.levels) - 1
    assert (ex.stop < last).any() and (ex.stop == last).any(), (ex.tol, ex.stop)


# ---- the GPU run -----------------------------------------------------------------------

class Run:
    """A context with its tile and frame buffers; level() renders one level and assembles."""

    def __init__(self, scenes, which, p):
        import torch
        self.keep, self.view, self.cam = E.scene_of(scenes, which)
        self.p = p
        self.ctx = z.RenderContext(self.view, p)
        self.tiles = torch.zeros(self.ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
        self.dev_frame = torch.zeros(p.height * p.width * 3, dtype=torch.float32, device="cuda")

    def begin(self, tol, first, p=None):
        self.p = p or self.p
        self.tiles.zero_()
        self.ctx.adapt_begin(self.cam, self.p, tol, first)

    def frame(self):
        import torch
        self.ctx.assemble(self.p, self.tiles.data_ptr(), self.dev_frame.data_ptr())
        torch.cuda.synchronize()
        return self.dev_frame.cpu().numpy().reshape(self.p.height, self.p.width, 3)

    def level(self):
        info = self.ctx.adapt_level(self.tiles.data_ptr())
        return info, self.frame()

    def close(self):
        self.ctx.close()


def check_run(scenes, which, p, first, ex, run=None):
    """Every level of the GPU run against ex: the assembled frame bit for bit, the sample map,
    the level's tile counts and samples; the run ends where the expected one does.
    Returns (last frame, stats, infos)."""
    own = run is None
    run = run or Run(scenes, which, p)
    pix = in_frame_pixels(p)
    try:
        run.begin(ex.tol, first, p)
        infos, done = [], 0
        for k, ((rendered, after), comp) in enumerate(zip(ex.steps, ex.frames)):
            info, img = run.level()
            print(f"{which} tol {ex.tol} level {k}: {info}")
            P.assert_bit_exact(img, comp)
            np.testing.assert_array_equal(run.ctx.adapt_samples(), ex.samples(k))
            assert (info["level_samples"], info["tiles_rendered"], info["tiles_active_after"]) == \
                (ex.levels[k], rendered, after if k + 1 < len(ex.levels) else 0)
            assert info["samples_rendered"] == int(pix[ex.stop >= k].sum()) * (ex.levels[k] - done)
            done = ex.levels[k]
            infos.append(info)
        with pytest.raises(z.ZrtError) as e:
            run.level()
        assert e.value.code == E_INVALID
        st = run.ctx.stats()
        assert st["samples_processed"] == int((pix * ex.samples(len(ex.steps) - 1).astype(np.uint64)).sum())
        assert st["pixels_processed"] == int(pix.sum())
        return img, st, infos
    finally:
        if own:
            run.close()


def check_uniform(scenes, which, p, run, st, spp):
    """A run that left every tile at spp: the oracle's Progress counters (and scanline rows) at spp."""
    _, rs, rrows = E.oracle_frame(scenes, which, dataclasses.replace(p, samples_per_pixel=spp))
    for k in P.COUNTERS:
        assert st[k] == rs[k], (k, spp)
    if p.flags & SCANLINES:
        np.testing.assert_array_equal(run.ctx.scanlines(p.height), rrows)


def level_params(loop, prng, monkeypatch, cap, flags=0):
    p = E.frame_params(12, E.PRNGS[prng], spp=cap, chunk=3)
    p = dataclasses.replace(p, bounded_volume_hierarchy=loop not in E.LIST_LOOPS)
    p = E.set_edge_loop(monkeypatch, loop, p)
    return dataclasses.replace(p, flags=p.flags | flags)


# ---- 1. decisions and pixels against the oracle ------------------------------------------

@pytest.mark.parametrize("name", SCENES + ["wraps"])
def test_decisions_and_pixels(scenes, name, monkeypatch):
    """24 x 24, depth 12, chunk 3, first 3, cap 48: levels 3, 6, 12, 24, 48.  The tolerance of
    2^-k with the most distinct stop levels gives a mixed map; after every level the frame is
    the composite of the oracle's frames, the sample map and the level's counts are the
    rule's, and the run ends where the rule ends it."""
    p = level_params("lockstep", "xoroshiro", monkeypatch, 48)
    ex = expected_run(scenes, name, p, 3)
    assert ex.levels == [3, 6, 12, 24, 48]
    assert_mixed(ex)
    img, st, infos = check_run(scenes, name, p, 3, ex)
    assert st["sampling_loop"] == 3
    assert all(i["schedule_ms"] == 0 for i in infos) and all(i["render_ms"] > 0 for i in infos)


# ---- 2. every loop, both PRNGs -----------------------------------------------------------

@pytest.mark.parametrize("prng", list(E.PRNGS))
@pytest.mark.parametrize("loop", E.BVH_LOOPS + E.LIST_LOOPS)
@pytest.mark.parametrize("name", SCENES)
def test_every_loop(scenes, name, loop, prng, monkeypatch):
    """Case 1 at cap 24 (levels 3, 6, 12, 24) through every sampling loop: each loop's
    tile_order read and total_work bound must honour a shrunken active list."""
    p = level_params(loop, prng, monkeypatch, 24)
    ex = expected_run(scenes, name, p, 3)
    assert_mixed(ex)
    _, st, _ = check_run(scenes, name, p, 3, ex)
    assert st["sampling_loop"] == E.LOOPS[loop][3]


# ---- 3. degenerate tolerances -------------------------------------------------------------

@pytest.mark.parametrize("flags", [0, SCANLINES], ids=["plain", "scanlines"])
@pytest.mark.parametrize("name", ["glass-inside", "wraps"])
def test_degenerate_tolerances(scenes, name, flags, monkeypatch):
    """tolerance 1e30: every tile stops at the first decision (6 samples), and the counters and
    scanline rows are the oracle's at 6 spp.  tolerance 0: whatever the rule says (a tile of
    unchanged pixels may stop); where that map is uniform, the oracle's counters again, and at
    the cap z.render's frame and counters."""
    p = level_params("lockstep", "xoroshiro", monkeypatch, 24, flags)
    run = Run(scenes, name, p)
    try:
        ex = expected_run(scenes, name, p, 3, tol=1e30)
        assert (ex.stop == 1).all() and len(ex.steps) == 2
        img, st, _ = check_run(scenes, name, p, 3, ex, run)
        check_uniform(scenes, name, p, run, st, 6)
        ex0 = expected_run(scenes, name, p, 3, tol=0.0)
        img, st, _ = check_run(scenes, name, p, 3, ex0, run)
        spp = set(ex0.samples(len(ex0.steps) - 1).tolist())
        if len(spp) == 1:
            check_uniform(scenes, name, p, run, st, spp.pop())
        if (ex0.stop == len(ex0.levels) - 1).all():
            _, view, cam = E.scene_of(scenes, name)
            full, fs = z.render(view, cam, p)
            assert P.same_bits(img, full).all()
            for k in P.COUNTERS:
                assert fs[k] == st[k], k
    finally:
        run.close()


def test_single_level_is_render(scenes, monkeypatch):
    """first >= cap: one level, no decision, z.render's frame and counters."""
    p = level_params("lockstep", "xoroshiro", monkeypatch, 12, SCANLINES)
    ex = expected_run(scenes, "wraps", p, 12, tol=1e30)
    assert ex.levels == [12] and ex.steps == [(9, 0)]
    run = Run(scenes, "wraps", p)
    try:
        img, st, _ = check_run(scenes, "wraps", p, 12, ex, run)
        check_uniform(scenes, "wraps", p, run, st, 12)
        _, view, cam = E.scene_of(scenes, "wraps")
        full, fs = z.render(view, cam, p)
        assert P.same_bits(img, full).all()
        for k in P.COUNTERS:
            assert fs[k] == st[k], k
    finally:
        run.close()


# ---- 4. behind the scheduling probe --------------------------------------------------------

@pytest.mark.parametrize("name", SCENES + ["wraps"])
def test_behind_the_probe(scenes, name, monkeypatch):
    """24 x 24, chunk 24, first 24, cap 192 (levels 24 .. 192), the lockstep loop, scheduled:
    level 0 probes and the active list starts from the probe's order; frames and map as in
    case 1, and the probe's time on level 0 only."""
    p = E.set_edge_loop(monkeypatch, "lockstep", E.frame_params(12, spp=192, chunk=24))
    ex = expected_run(scenes, name, p, 24)
    assert ex.levels == [24, 48, 96, 192]
    assert_mixed(ex)
    _, st, infos = check_run(scenes, name, p, 24, ex)
    assert [i["schedule_ms"] > 0 for i in infos] == [True] + [False] * (len(infos) - 1)
    assert st["schedule_ms"] > 0 and st["render_ms"] > st["schedule_ms"]


# ---- 5. ragged edges --------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES + ["wraps"])
def test_ragged_edges(scenes, name, monkeypatch):
    """20 x 12: the tiles of the second row and column are partly off-frame (their off-frame
    lanes must not hold them active), and the pixels with x >= 12 stay 0; cap 20 with chunk 3
    makes the last level (12 .. 20) ragged."""
    p = E.set_edge_loop(monkeypatch, "lockstep", E.frame_params(12, w=20, h=12, spp=20, chunk=3))
    ex = expected_run(scenes, name, p, 3)
    assert ex.levels == [3, 6, 12, 20] and len(ex.stop) == 4
    assert_mixed(ex)
    img, st, _ = check_run(scenes, name, p, 3, ex)
    assert not img[:, 12:].any() and img[:, :12].any()


# ---- 6. two ranks on one GPU --------------------------------------------------------------

def test_two_ranks(scenes, monkeypatch):
    """world_size 2: each rank's run covers its own tiles (t = 2 lt + rank) and decides per
    tile, so its tiles and its sample map are the N = 1 run's for those tiles."""
    import torch
    p = level_params("lockstep", "xoroshiro", monkeypatch, 48)
    ex = expected_run(scenes, "wraps", p, 3)
    assert_mixed(ex)
    boxes = tile_boxes(p)
    for rank in (0, 1):
        pr = dataclasses.replace(p, rank=rank, world_size=2)
        mine = list(range(rank, len(boxes), 2))
        run = Run(scenes, "wraps", pr)
        try:
            run.ctx.adapt_begin(run.cam, pr, ex.tol, 3)
            k = 0
            while True:
                active = [t for t in mine if ex.stop[t] >= k]
                if k == len(ex.levels) or not active:
                    break
                info = run.ctx.adapt_level(run.tiles.data_ptr())
                torch.cuda.synchronize()
                assert info["tiles_rendered"] == len(active) and info["level_samples"] == ex.levels[k]
                np.testing.assert_array_equal(run.ctx.adapt_samples(), ex.samples(k)[mine])
                tiles = run.tiles.cpu().numpy().reshape(-1, 8, 8, 3)
                for lt, t in enumerate(mine):
                    x0, x1, y0, y1 = boxes[t]
                    want = np.zeros((8, 8, 3), np.float32)
                    want[:y1 - y0, :x1 - x0] = ex.frames[min(k, len(ex.frames) - 1)][y0:y1, x0:x1]
                    assert P.same_bits(tiles[lt], want).all(), (rank, k, t)
                k += 1
            with pytest.raises(z.ZrtError) as e:
                run.ctx.adapt_level(run.tiles.data_ptr())
            assert e.value.code == E_INVALID
        finally:
            run.close()


# ---- 7. counters in a mixed run -----------------------------------------------------------

@pytest.mark.parametrize("name", SCENES + ["wraps"])
def test_mixed_run_counters(scenes, name, monkeypatch):
    """A mixed run: samples_processed is the sum of in-frame pixels x samples over the expected
    map and pixels_processed the frame's (both in check_run); the STATS flavour counts
    rays_processed itself and it equals samples + reflections - recursion_depth_hits; the
    timed flavour reports the same numbers."""
    p = level_params("lockstep", "xoroshiro", monkeypatch, 48)
    ex = expected_run(scenes, name, p, 3)
    assert_mixed(ex)
    _, st, _ = check_run(scenes, name, p, 3, ex)
    ps = dataclasses.replace(p, flags=p.flags | z.ZRT_FLAG_STATS)
    _, ss, _ = check_run(scenes, name, ps, 3, ex)
    assert ss["node_visits"] > 0
    assert ss["rays_processed"] == ss["samples_processed"] + ss["reflections"] - ss["recursion_depth_hits"]
    for k in P.COUNTERS:
        assert st[k] == ss[k], k
    full = E.oracle_frame(scenes, name, p)[1]
    assert 0 < st["samples_processed"] < full["samples_processed"]
    assert 0 < st["rays_processed"] < full["rays_processed"]


# ---- 8. run state ---------------------------------------------------------------------

def test_run_state(scenes, monkeypatch):
    p = level_params("lockstep", "xoroshiro", monkeypatch, 24)
    ex = expected_run(scenes, "wraps", p, 3)
    run = Run(scenes, "wraps", p)
    try:
        with pytest.raises(z.ZrtError) as e:  # no live run
            run.level()
        assert e.value.code == E_INVALID and "no adaptive run" in str(e.value)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(z.ZrtError) as e:
                run.begin(bad, 3)
            assert e.value.code == E_INVALID
        run.begin(ex.tol, 3)
        run.level()
        with pytest.raises(z.ZrtError) as e:  # a level of a plain run is not this run's
            run.ctx.accum_pass(3, run.tiles.data_ptr())
        assert e.value.code == E_INVALID
        # a plain render ends the run
        run.ctx.render_tiles(run.cam, p, run.tiles.data_ptr())
        run.ctx.sync()
        with pytest.raises(z.ZrtError) as e:
            run.level()
        assert e.value.code == E_INVALID and "no adaptive run" in str(e.value)
        # adapt_begin after accum_begin, and the reverse: each restarts cleanly
        run.ctx.accum_begin(run.cam, p)
        run.ctx.accum_pass(6, run.tiles.data_ptr())
        with pytest.raises(z.ZrtError) as e:
            run.level()
        assert e.value.code == E_INVALID
        check_run(scenes, "wraps", p, 3, ex, run)
        run.ctx.accum_begin(run.cam, p)
        run.ctx.accum_pass(6, run.tiles.data_ptr())
        P.assert_bit_exact(run.frame(), E.oracle_frame(scenes, "wraps", dataclasses.replace(p, samples_per_pixel=6))[0])
        assert run.ctx.stats()["samples_processed"] == 24 * 24 * 6
        check_run(scenes, "wraps", p, 3, ex, run)
    finally:
        run.close()


def test_sticky_device_error(scenes, monkeypatch):
    """test_gpu_progressive's safe hook (scene 3, 128 x 128, depth 20, the STATS flavour told
    its row buffers hold nothing: the device check skips the access and raises the error
    flag), levels 2 and 4: the erroring level gives NaN tiles and the error, the rest of the
    run is refused with it, and a new run without the cap is exact again."""
    s = scenes(3)
    p = z.RenderParams(128, 128, 4, 20, flags=z.ZRT_FLAG_STATS, sample_chunk=2)
    monkeypatch.setenv("ZRT_POOL", "0")
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS", "2")
    run = Run(scenes, 3, p)
    try:
        monkeypatch.setenv("ZRT_DEBUG_ROW_CAP", "0")
        run.begin(0.0, 2)
        with pytest.raises(z.ZrtError, match="past its buffer") as e:
            run.level()
        assert e.value.code == E_UNSUPPORTED
        assert np.isnan(run.frame()).all()
        monkeypatch.delenv("ZRT_DEBUG_ROW_CAP")
        for call in (run.level, run.ctx.sync, run.ctx.stats):
            with pytest.raises(z.ZrtError, match="past its buffer") as e:
                call()
            assert e.value.code == E_UNSUPPORTED
        assert np.isnan(run.frame()).all()
        run.begin(0.0, 4)  # one level: the frame of z.render
        _, img = run.level()
        ref, rs = z.render(s, s.camera, p)
        assert P.same_bits(img, ref).all() and np.isfinite(img).all()
        assert run.ctx.stats()["rays_processed"] == rs["rays_processed"]
    finally:
        run.close()


# ---- 9. front ends --------------------------------------------------------------------

def test_render_adaptive(scenes, monkeypatch):
    """z.render_adaptive on case 1: the last composite, the map expanded to pixels, one
    callback per level with the composite of that level; a callback that stops the run."""
    p = level_params("lockstep", "xoroshiro", monkeypatch, 48)
    ex = expected_run(scenes, "wraps", p, 3)
    assert_mixed(ex)
    _, view, cam = E.scene_of(scenes, "wraps")
    seen = []
    img, samples, st, infos = z.render_adaptive(view, cam, p, ex.tol, 3,
                                                on_level=lambda im, info: seen.append(im.copy()) and False)
    assert len(infos) == len(seen) == len(ex.steps)
    for got, comp in zip(seen, ex.frames):
        P.assert_bit_exact(got, comp)
    P.assert_bit_exact(img, ex.frames[-1])
    want = np.zeros((p.height, p.width), np.uint32)
    final = ex.samples(len(ex.steps) - 1)
    for t, (x0, x1, y0, y1) in enumerate(tile_boxes(p)):
        want[y0:y1, x0:x1] = final[t]
    np.testing.assert_array_equal(samples, want)
    assert st["samples_processed"] == int(want.astype(np.uint64).sum())
    assert [i["level_samples"] for i in infos] == ex.levels[:len(ex.steps)]
    calls = []
    img, samples, st, infos = z.render_adaptive(view, cam, p, ex.tol, 3,
                                                on_level=lambda im, info: calls.append(info) or len(calls) == 2)
    assert len(infos) == 2
    P.assert_bit_exact(img, ex.frames[1])


def test_cli_adaptive(scenes, tmp_path):
    """zrt-raytrace 32 32 128 5 1 out.png with ZRT_ADAPTIVE_TOL and ZRT_ADAPTIVE_FIRST=32
    (levels 32, 64, 128 of the three balls): the PNG is the composite's, the map PNG is
    samples / cap in grey, one Level line per level."""
    p = z.RenderParams(32, 32, 128, 5, seed=42, sample_chunk=0)
    ex = expected_run(scenes, 1, p, 32)
    assert ex.levels == [32, 64, 128]
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    env = {k: v for k, v in os.environ.items() if k not in ("ZRT_PASS_SAMPLES", "ZRT_DEVICES")}
    env.update(ZRT_ADAPTIVE_TOL=repr(ex.tol), ZRT_ADAPTIVE_FIRST="32", ZRT_ADAPTIVE_MAP=str(tmp_path / "map.png"))
    r = subprocess.run([exe, "32", "32", "128", "5", "1", str(tmp_path / "out.png")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert len([ln for ln in r.stderr.splitlines() if ln.startswith("Level: ")]) == len(ex.steps)
    # the scanline lines once, at the end, from the accumulated rows: a row's samples are its tiles' own
    rows = [ln for ln in r.stderr.splitlines() if ln.startswith("Scanline: ")]
    total = int((in_frame_pixels(p) * ex.samples(len(ex.steps) - 1).astype(np.uint64)).sum())
    assert len(rows) == 32 and rows[-1].startswith(f"Scanline: 32/32 Pixels: 1024 Samples: {total} ")
    assert f"  Total samples:         {total}" in r.stderr.splitlines()
    z.write_png(str(tmp_path / "want.png"), ex.frames[-1])
    assert (tmp_path / "out.png").read_bytes() == (tmp_path / "want.png").read_bytes()
    grey = np.zeros((32, 32, 3), np.float32)
    final = ex.samples(len(ex.steps) - 1)
    for t, (x0, x1, y0, y1) in enumerate(tile_boxes(p)):
        grey[y0:y1, x0:x1] = np.float32(final[t]) / np.float32(128)
    z.write_png(str(tmp_path / "want_map.png"), grey)
    assert (tmp_path / "map.png").read_bytes() == (tmp_path / "want_map.png").read_bytes()
    r = subprocess.run([exe, "32", "32", "128", "5", "1", str(tmp_path / "both.png")],
                       env={**env, "ZRT_PASS_SAMPLES": "32"}, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "ZRT_ADAPTIVE_TOL" in r.stderr and not (tmp_path / "both.png").exists()

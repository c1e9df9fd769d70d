"""Launch-configuration edges of the sampling loops against the oracle.

The parity suite (test_gpu_parity.py) is wide on geometry; this file is about
what the launch decision (planner.cpp plan_launch, reported with no device by
zrt_debug_launch_plan) and the loops' row bookkeeping do at their edges:

* max_depth 0 .. 3 in every loop (no loop shades at 0; no attenuation row is
  pushed below 2);
* the boundary between the attenuation rows in LDS and those in global memory
  (ZRT_ATT_LDS_ROWS=k, max_depth - 1 at k, k + 1 and k + 2);
* the 16-bit traversal stack's global overflow rows (ZRT_STACK_LDS_ROWS16) in
  the lockstep, wavefront and path-pool loops, in zrt_trace and in the
  scheduling probe;
* the xoshiro256 generator through the BVH loops (a wider parked lane state,
  other LDS offsets, the pool's per-path generator), at depth and through the
  scheduling probe.

Every case compares with the oracle bit for bit: the image, the Progress counters
and the per-scanline rows; every timed render is followed by the STATS flavour,
which must give the same bits.  A counter that must be > 0 is preceded by the
oracle-side condition that makes it so, so that a case no path exercises fails.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O

import many_materials as M
import shading_scenes as SH
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

K_ATT_WRITES, K_STACK_OVF_WRITES = 28, 30  # debug_counters slots (render.hip kAttWrites, kStackOvfWrites)
PRNGS = {"xoroshiro": z.ZRT_PRNG_XOROSHIRO128, "xoshiro": z.ZRT_PRNG_XOSHIRO256}

# loop -> (environment, traversal, flags, zrt_stats.sampling_loop at max_depth >= 1)
FAST, BINARY, REFERENCE = z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE
LOOPS = {
    "lockstep": ({"ZRT_WF": "0", "ZRT_POOL": "0"}, FAST, 0, 3),
    "wavefront": ({"ZRT_WF": "1", "ZRT_POOL": "0"}, FAST, 0, 4),
    "pool": ({"ZRT_WF": "0", "ZRT_POOL": "1"}, FAST, 0, 5),
    # (the guard alone asks for the pool: ZRT_POOL stays 0)
    "pool-guard": ({"ZRT_WF": "0", "ZRT_POOL": "0"}, FAST, z.ZRT_FLAG_GUARD, 5),
    "pool-qnodes": ({"ZRT_WF": "0", "ZRT_POOL": "1", "ZRT_QNODES": "1"}, FAST, 0, 5),
    "binary": ({}, BINARY, 0, 1),
    "reference": ({}, REFERENCE, 0, 2),
    "list-items": ({"ZRT_LIST_LANES": "1"}, FAST, 0, 6),
    "list-wave": ({"ZRT_LIST_LANES": "0"}, FAST, 0, 0),
}
BVH_LOOPS = ["lockstep", "wavefront", "pool", "pool-guard", "pool-qnodes", "binary", "reference"]
LIST_LOOPS = ["list-items", "list-wave"]
STACK_LOOPS = ["lockstep", "wavefront", "pool", "pool-qnodes"]  # the FAST loops: a stack with overflow rows


def set_edge_loop(monkeypatch, loop, p):
    """Force one sampling loop; returns p with the loop's traversal and flags."""
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES"):
        monkeypatch.delenv(k, raising=False)
    env, trav, flags, _ = LOOPS[loop]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return dataclasses.replace(p, traversal=trav, flags=flags)


# ---- scenes and the oracle's frames of them ------------------------------------------

_MM = {}


def scene_of(scenes, which):
    """(object to keep alive, zrt_scene pointer, camera) of a reference scene index,
    "mm": the many-materials grid whose table fits the lockstep loop's LDS share, or a
    name of tests/shading_scenes.py."""
    if which in SH.NAMES:
        return SH.get(which)
    if which == "mm":
        if not _MM:
            _MM["scene"] = M.many_materials_scene(M.N_SIDE_LOCKSTEP)
            _MM["camera"] = M.camera(M.N_SIDE_LOCKSTEP)
        import ctypes as C
        return _MM["scene"], C.pointer(_MM["scene"]), _MM["camera"]
    s = scenes(which)
    return s, s.view, s.camera


_ORACLE = {}  # (scene, width, height, spp, max_depth, prng, seed, chunk, bvh) -> (image, stats, scanline rows)


def oracle_frame(scenes, which, p):
    """The oracle's frame, computed once and shared (never written to).  The loop,
    the traversal and the flags change nothing the oracle computes."""
    key = (which, p.width, p.height, p.samples_per_pixel, p.max_depth, p.prng, p.seed, p.sample_chunk,
           p.bounded_volume_hierarchy)
    if key not in _ORACLE:
        _, view, cam = scene_of(scenes, which)
        plain = z.RenderParams(p.width, p.height, p.samples_per_pixel, p.max_depth, prng=p.prng, seed=p.seed,
                               sample_chunk=p.sample_chunk, bounded_volume_hierarchy=p.bounded_volume_hierarchy)
        img, st, rows = O.render_scanlines(view, cam, plain)
        img.setflags(write=False)
        rows.setflags(write=False)
        _ORACLE[key] = (img, st, rows)
    return _ORACLE[key]


def depth_hits(scenes, which, p, depth):
    """The oracle's recursion_depth_hits of p's frame at another max_depth: the paths
    that scatter `depth` times."""
    return oracle_frame(scenes, which, dataclasses.replace(p, max_depth=depth))[1]["recursion_depth_hits"]


def check_frame(scenes, which, p, scanlines=True):
    """Timed flavour (with the scanline rows) and STATS flavour of p against the
    oracle: image bit for bit, Progress counters, rows.  Returns (gpu stats, oracle stats)."""
    _, view, cam = scene_of(scenes, which)
    ref, rs, rrows = oracle_frame(scenes, which, p)
    if scanlines:
        gpu, gs, rows = z.render_progress(view, cam, p)
        np.testing.assert_array_equal(rows, rrows)
    else:
        gpu, gs = z.render(view, cam, p)
    P.assert_bit_exact(gpu, ref)
    for k in P.COUNTERS:
        assert gs[k] == rs[k], k
    gpu2, gs2 = z.render(view, cam, dataclasses.replace(p, flags=p.flags | z.ZRT_FLAG_STATS))
    assert P.same_bits(gpu, gpu2).all(), "the STATS flavour renders other bits"
    for k in P.COUNTERS:
        assert gs2[k] == rs[k], k
    assert gs2["sampling_loop"] == gs["sampling_loop"]
    return gs, rs


def stats_counters(scenes, which, p):
    """debug_counters of a STATS launch of p from a context."""
    import torch
    keep, view, cam = scene_of(scenes, which)
    ps = dataclasses.replace(p, flags=p.flags | z.ZRT_FLAG_STATS)
    ctx = z.RenderContext(keep if which != "mm" else view, ps)
    try:
        buf = torch.zeros(ctx.tile_count(ps) * 64 * 3, dtype=torch.float32, device="cuda")
        ctx.render_tiles(cam, ps, buf.data_ptr())
        ctx.sync()
        return ctx.debug_counters(32)
    finally:
        ctx.close()


def frame_params(depth, prng=z.ZRT_PRNG_XOROSHIRO128, w=24, h=24, spp=4, chunk=3, seed=42):
    return z.RenderParams(w, h, spp, depth, prng=prng, seed=seed, sample_chunk=chunk)


# ---- 1. shallow depths in every loop ---------------------------------------------------

@pytest.mark.parametrize("prng", list(PRNGS))
@pytest.mark.parametrize("max_depth", [0, 1, 2, 3])
@pytest.mark.parametrize("loop", BVH_LOOPS + LIST_LOOPS)
def test_shallow_depths_every_loop(scenes, loop, max_depth, prng, monkeypatch):
    """max_depth 0 .. 3 in every sampling loop (scene 4 for the BVH loops, the seven
    spheres for the list loops), both generators, scanline rows included.  At 0 the
    frame is black, every sample ends at the depth limit, and no loop written for
    max_depth >= 1 runs: ZRT_WF=1, ZRT_POOL=1 and the guard keep the lockstep loop."""
    which = 1 if loop in LIST_LOOPS else 4
    p = set_edge_loop(monkeypatch, loop, frame_params(max_depth, PRNGS[prng]))
    gs, rs = check_frame(scenes, which, p)
    want = LOOPS[loop][3]
    if max_depth == 0:
        assert rs["recursion_depth_hits"] == rs["samples_processed"] == 24 * 24 * 4 and rs["rays_processed"] == 0
        assert gs["recursion_depth_hits"] == gs["samples_processed"]
        assert not oracle_frame(scenes, which, p)[0].any()
        if want in (4, 5):
            want = 3
    else:
        assert rs["recursion_depth_hits"] > 0  # (some path reaches the limit: not vacuous)
    assert gs["sampling_loop"] == want
    _, view, _ = scene_of(scenes, which)
    assert z.debug_launch_plan(view, p)["sampling_loop"] == want


# ---- 3. the LDS-to-global boundary of the attenuation rows -----------------------------

ATT_CASES = [(which, loop) for which in ("mm", 4) for loop in BVH_LOOPS if (which, loop) != ("mm", "pool-guard")]
ATT_CASES += [(1, loop) for loop in LIST_LOOPS]  # (the grid has no triangle: nothing to guard)


@pytest.mark.parametrize("prng,k,extra", [("xoroshiro", k, e) for k in (0, 1, 2, 3) for e in (1, 2, 3)] +
                         [("xoshiro", 2, e) for e in (1, 2, 3)])
@pytest.mark.parametrize("which,loop", ATT_CASES, ids=[f"{w}-{l}" for w, l in ATT_CASES])
def test_attenuation_row_boundary(scenes, which, loop, prng, k, extra, monkeypatch):
    """ZRT_ATT_LDS_ROWS=k with max_depth D = k + 1, k + 2, k + 3: rows 0 .. D-2 are
    pushed, the first att_rows of them (k capped by the loop's own limit and its LDS
    room: zrt_debug_launch_plan reports it) live in LDS and the rest in global memory,
    so D - 1 sits at att_rows - 1, att_rows and att_rows + 1 where the cap does not
    bite.  Parity with the oracle, and the STATS launch's count of global attenuation
    writes (kAttWrites): 0 when D - 1 <= att_rows, > 0 beyond - there the oracle shows
    that some path scatters at row att_rows (its depth-limit hits at max_depth
    att_rows + 1 are > 0) and that some path ends after exactly D - 1 scatters (more
    hits at D - 1 than at D), whose product reads every row."""
    D = k + extra
    monkeypatch.setenv("ZRT_ATT_LDS_ROWS", str(k))
    p = set_edge_loop(monkeypatch, loop, frame_params(D, PRNGS[prng]))
    _, view, _ = scene_of(scenes, which)
    plan = z.debug_launch_plan(view, p)
    att_rows = plan["att_rows"]
    assert att_rows <= min(k, D - 1)
    assert plan["att_rows_per_path"] >= max(1, D - 1 - att_rows)
    if which == "mm" and loop == "lockstep":
        assert (plan["kmode"], plan["mats_in_lds"]) == (3, 1)  # (the table fits: the lockstep loop itself)
    gs, rs = check_frame(scenes, which, p)
    assert gs["sampling_loop"] == plan["sampling_loop"] == LOOPS[loop][3]
    dc = stats_counters(scenes, which, p)
    print(f"{which} {loop} k={k} D={D} att_rows={att_rows} kAttWrites={dc[K_ATT_WRITES]}")
    if D - 1 <= att_rows:
        assert dc[K_ATT_WRITES] == 0
    else:
        assert depth_hits(scenes, which, p, att_rows + 1) > 0
        assert depth_hits(scenes, which, p, D - 1) > depth_hits(scenes, which, p, D)
        assert dc[K_ATT_WRITES] > 0, "no attenuation row reached global memory"


# ---- 4. the 16-bit stack's global overflow rows ------------------------------------------

def deep_traversal(rs, rows):
    """Oracle-side condition of a stack that outgrows `rows` LDS rows: the reference
    traversal visits, on average, more nodes per ray than a descent `rows` + 2 levels
    deep with both children opened at each - rays do go deep into the tree, with
    farther siblings waiting on the stack (not a frame of misses)."""
    return rs["used_bvh"] == 1 and rs["node_visits"] > 2 * (rows + 2) * rs["rays_processed"] > 0


@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("loop", STACK_LOOPS)
@pytest.mark.parametrize("which", [2, 3])
def test_stack16_overflow_rows(scenes, which, loop, rows, monkeypatch):
    """ZRT_STACK_LDS_ROWS16 keeps the 16-bit stack of these trees (< 65 536 nodes)
    and leaves 1, 2 or 4 of its rows in LDS: most pushes and pops of wide_iter /
    wide_iter_q go through the 16-bit global rows, in the lockstep, wavefront and
    path-pool loops (full and compressed nodes).  The oracle's frame, and overflow
    writes counted (kStackOvfWrites)."""
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS16", str(rows))
    p = set_edge_loop(monkeypatch, loop, frame_params(8, w=24, h=16))
    _, view, _ = scene_of(scenes, which)
    plan = z.debug_launch_plan(view, p)
    assert (plan["stk16"], plan["stack_rows"]) == (1, rows), plan
    assert plan["stack_depth"] > rows and plan["ovf_bytes_per_lane"] == 2 * (plan["stack_depth"] - rows)
    assert plan["qnodes"] == (1 if loop == "pool-qnodes" else 0)
    gs, rs = check_frame(scenes, which, p)
    assert gs["sampling_loop"] == LOOPS[loop][3]
    dc = stats_counters(scenes, which, p)
    print(f"scene {which} {loop} rows={rows} kStackOvfWrites={dc[K_STACK_OVF_WRITES]} "
          f"oracle nodes/ray={rs['node_visits'] / rs['rays_processed']:.1f}")
    assert deep_traversal(rs, rows)
    assert dc[K_STACK_OVF_WRITES] > 0, "no stack entry reached the global rows"


@pytest.mark.parametrize("qnodes", [False, True], ids=["full", "compressed"])
@pytest.mark.parametrize("rows", [1, 2, 4])
def test_stack16_overflow_rows_trace(scenes, rows, qnodes, monkeypatch):
    """zrt_trace on test_trace_mesh_rays_bit_exact's rays for the bunny scene with the
    16-bit stack on its global rows (the vertex rays take the order-hazard replay
    there too), over the full and the compressed nodes."""
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS16", str(rows))
    if qnodes:
        monkeypatch.setenv("ZRT_QNODES", "1")
    s = scenes(2)
    if (2, "rays") not in _ORACLE:
        origins, dirs = P.mesh_rays(s, 2)
        _ORACLE[2, "rays"] = (origins, dirs) + O.trace(s.view, True, origins, dirs)
    origins, dirs, t_ref, p_ref = _ORACLE[2, "rays"]
    assert (p_ref >= 0).mean() > 0.3
    t, p = z.trace(s, z.RenderParams(1, 1, 1, 1, traversal=FAST), origins, dirs)
    P.assert_same_hits(t, p, t_ref, p_ref)


@pytest.mark.parametrize("loop", STACK_LOOPS)
def test_stack16_overflow_rows_behind_probe(scenes, loop, monkeypatch):
    """The scheduling probe (spp >= 128: a lockstep launch with an LDS plan of its
    own) in front of each FAST loop, both on 16-bit global stack rows: the probe's
    plan sees ZRT_STACK_LDS_ROWS16 too and shares the render launch's buffer."""
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS16", "2")
    p = set_edge_loop(monkeypatch, loop, frame_params(6, spp=128, chunk=0))
    _, view, _ = scene_of(scenes, 2)
    plan = z.debug_launch_plan(view, p)
    assert (plan["stk16"], plan["stack_rows"]) == (1, 2), plan
    gs, rs = check_frame(scenes, 2, p, scanlines=False)
    assert gs["schedule_ms"] > 0 and gs["sampling_loop"] == LOOPS[loop][3]


# ---- 5. xoshiro256 through the BVH loops ---------------------------------------------------

@pytest.mark.parametrize("loop", ["lockstep", "wavefront", "pool", "pool-guard", "pool-qnodes"])
def test_xoshiro_bvh_loops_at_depth(scenes, loop, monkeypatch):
    """ZRT_PRNG_XOSHIRO256 (a 256-bit state: other LaneState words parked in LDS
    across each traversal, other LDS offsets, the pool's generator per path through
    its compaction) on scene 4 at depth 20, 24 spp in chunks of 7, scanline rows
    included: the oracle's frame in every FAST loop."""
    p = set_edge_loop(monkeypatch, loop, frame_params(20, z.ZRT_PRNG_XOSHIRO256, spp=24, chunk=7))
    gs, rs = check_frame(scenes, 4, p)
    assert gs["sampling_loop"] == LOOPS[loop][3]
    assert rs["rays_processed"] > rs["samples_processed"]  # (paths scatter: rays beyond the camera rays)


@pytest.mark.parametrize("schedule", [True, False], ids=["probe", "no-schedule"])
@pytest.mark.parametrize("loop", ["lockstep", "pool"])
def test_xoshiro_through_the_probe(scenes, loop, schedule, monkeypatch):
    """The scheduling probe with xoshiro's lane state (scene 2 at 128 spp, depth 6),
    in front of the lockstep loop (which then takes its interval from the probe) and
    of the path pool; and the same frames unscheduled."""
    p = set_edge_loop(monkeypatch, loop, frame_params(6, z.ZRT_PRNG_XOSHIRO256, spp=128, chunk=0))
    if not schedule:
        p = dataclasses.replace(p, flags=p.flags | z.ZRT_FLAG_NO_SCHEDULE)
    gs, rs = check_frame(scenes, 2, p, scanlines=False)
    assert (gs["schedule_ms"] > 0) == schedule
    assert gs["sampling_loop"] == LOOPS[loop][3]

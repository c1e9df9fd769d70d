"""Adaptive and progressive runs over 1089 tiles: past a wave, a block and a round.

The runs of test_gpu_adaptive.py and test_gpu_progressive.py cover 9 tiles.  At that size
compact_kernel packs one wave of one round, accumulate_kernel and resolve_kernel launch 3
blocks into 3 of their 64 metric shards, and no wave of a level or a pass fetches a second
unit from the work counter.  Here the frame is 264 x 264: 33 x 33 = 1089 tiles = 1024 + 65,
so an active list spans two rounds of the compaction, a level's resolve is 273 blocks
wrapping round the shards four times, and the last level and the last pass hold more units
than the launch can have waves - every wave goes back to the counter, through the shrunken
list and with the pass's key offset.

The reference is the CPU oracle alone: test_gpu_adaptive's expected_run / check_run and
test_gpu_progressive's check_prefixes on test_gpu_loop_edges's shared frames (the four
frames of "wraps" at 3, 6, 12 and 24 samples serve the adaptive runs of both loops and every
prefix of the progressive ones).  What the input must look like for the scale-dependent
code to run is computed from the oracle's stop map and asserted before the GPU is asked.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z

import test_gpu_adaptive as A
import test_gpu_loop_edges as E
import test_gpu_progressive as G

pytestmark = pytest.mark.gpu

SIDE, TILES, ROUND = 264, 33 * 33, 1024  # ROUND: compact_kernel's block, kCompactBlock
FIRST, CAP, LEVELS = 3, 24, [3, 6, 12, 24]
PASSES = (3, 3, 6, 12)  # every prefix is one of LEVELS
LOOPS = ["lockstep", "pool"]


def scale_params(loop, monkeypatch, flags=0):
    """264 x 264, depth 12, seed 42, xoroshiro, one sample per chunk, cap 24."""
    p = E.set_edge_loop(monkeypatch, loop, E.frame_params(12, w=SIDE, h=SIDE, spp=CAP, chunk=1))
    return dataclasses.replace(p, flags=p.flags | flags)


def most_waves():
    """The most waves a launch can have: the grid is at most 8 blocks per CU (size_frame caps
    the occupancy there) of 4 waves each."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4


def round_counts(ex):
    """From the oracle's stop map alone.  Level 0 decides nothing and the run is not scheduled
    (cap < 128), so the list level 1 compacts is the identity: position = tile.  Returns
    ((frozen, surviving) after level 1 among positions 0 .. 1023, the same among positions
    1024 .. 1088, survivors of level 1 that freeze after level 2, tiles that reach the cap)."""
    assert ex.levels == LEVELS and len(ex.stop) == TILES
    frozen = ex.stop == 1
    first, second = frozen[:ROUND], frozen[ROUND:]
    return ((int(first.sum()), int((~first).sum())), (int(second.sum()), int((~second).sum())),
            int((ex.stop == 2).sum()), int((ex.stop == 3).sum()))


def check_level_metrics(ex, infos):
    """changed_pixels and max_abs_change of every level against numpy on consecutive composite
    frames (zeros before level 0): a frozen tile shows the same pixels in both, so the frame's
    difference is the rendered tiles'.  Summed by the host over resolve_kernel's shards."""
    prev, done = np.zeros_like(ex.frames[0]), 0
    for k, (info, comp) in enumerate(zip(infos, ex.frames)):
        n = ex.levels[k] - done
        G.check_metrics(dict(info, samples_done=info["level_samples"], pass_samples=n), comp, prev, n, ex.levels[k])
        prev, done = comp, ex.levels[k]
    assert len(infos) == len(ex.frames) == len(LEVELS)
    assert infos[0]["changed_pixels"] > 0 and infos[-1]["changed_pixels"] > 0


# ---- an adaptive run whose lists span two rounds ------------------------------------------

@pytest.mark.parametrize("loop", LOOPS)
def test_adaptive_wraps_two_rounds(scenes, loop, monkeypatch):
    """"wraps" at tolerance 2^-10.  The oracle's stop map: after level 1, 41 tiles freeze among
    list positions 0 .. 1023 and 9 among 1024 .. 1088 (kept and dropped entries on both sides
    of the round boundary); 1039 survive, so level 2's list spans two rounds as well, and 18 of
    them freeze there; 1021 reach the cap, whose level has 1021 x 12 = 12 252 units, more than
    the launch can have waves (8192 on 256 CUs).  Every level's frame, sample map and counts
    against the oracle (check_run), and the level's metrics, which 273 blocks of resolve_kernel
    add into 64 shards."""
    p = scale_params(loop, monkeypatch)
    ex = A.expected_run(scenes, "wraps", p, FIRST, tol=2.0 ** -10)
    A.assert_mixed(ex)
    (f1, s1), (f2, s2), freeze2, at_cap = round_counts(ex)
    print(f"wraps: level 1 freezes {f1} + {f2}, keeps {s1} + {s2}; level 2 freezes {freeze2}; {at_cap} reach the cap")
    assert (f1, s1, f2, s2, freeze2, at_cap) == (41, 983, 9, 56, 18, 1021)
    assert s1 + s2 > ROUND
    assert at_cap * (CAP - LEVELS[-2]) > most_waves()
    assert ex.steps == [(1089, 1089), (1089, 1039), (1039, 1021), (1021, 0)]
    _, st, infos = A.check_run(scenes, "wraps", p, FIRST, ex)
    assert st["sampling_loop"] == E.LOOPS[loop][3]
    check_level_metrics(ex, infos)


def test_adaptive_bubbles_mixed_rounds(scenes, monkeypatch):
    """"bubbles" at tolerance 2^-2, the lockstep loop: a far more mixed map, with another
    survivor pattern in each round of the first compaction - 540 freeze and 484 survive among
    positions 0 .. 1023, 55 freeze and 10 survive among 1024 .. 1088 - and 187 of the 494
    survivors freeze after level 2."""
    p = scale_params("lockstep", monkeypatch)
    ex = A.expected_run(scenes, "bubbles", p, FIRST, tol=2.0 ** -2)
    A.assert_mixed(ex)
    (f1, s1), (f2, s2), freeze2, at_cap = round_counts(ex)
    print(f"bubbles: level 1 freezes {f1} + {f2}, keeps {s1} + {s2}; level 2 freezes {freeze2}; {at_cap} reach the cap")
    assert (f1, s1, f2, s2, freeze2, at_cap) == (540, 484, 55, 10, 187, 307)
    _, st, infos = A.check_run(scenes, "bubbles", p, FIRST, ex)
    assert st["sampling_loop"] == 3
    check_level_metrics(ex, infos)


# ---- a progressive run over the same frame ---------------------------------------------

@pytest.mark.parametrize("loop", LOOPS)
def test_progressive_wraps(scenes, loop, monkeypatch):
    """The same frame in passes of 3, 3, 6 and 12 samples with the scanline rows: every prefix
    is a frame the adaptive run asked the oracle for.  The last pass has 1089 x 12 = 13 068
    units, more than the launch can have waves.  Frames, Progress counters, scanline rows and
    the pass metrics - accumulate_kernel's, from 273 blocks in 64 shards - against the oracle
    (check_prefixes)."""
    p = scale_params(loop, monkeypatch, z.ZRT_FLAG_SCANLINES)
    assert np.cumsum(PASSES).tolist() == LEVELS
    assert TILES * PASSES[-1] > most_waves()
    _, st, infos = G.check_prefixes(scenes, "wraps", p, PASSES)
    assert st["sampling_loop"] == E.LOOPS[loop][3]
    assert [i["schedule_ms"] for i in infos] == [0.0] * len(PASSES)  # (cap < 128: tile order)
    assert all(i["changed_pixels"] > 0 for i in infos)

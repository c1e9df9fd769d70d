"""The lean lockstep kernel against the general one and the oracle.

render.hip compiles the timed lockstep FAST kernel a second time for scenes of
solid-colour Lambertian and metal materials (render.hip struct Lean); the host launches it
where plan_launch and the camera allow it, and ZRT_LEAN=0 keeps the general
kernel.  Every case here renders with ZRT_LEAN=1 and with ZRT_LEAN=0, the timed
flavour and the STATS flavour (always the general kernel) of each, and asks of
all of them the oracle's frame bit for bit and its Progress counters;
zrt_debug_lean_kernel says which kernel the timed launch takes.

Frames are tiny (24 x 24 x 4, chunk 3, seed 42, as tests/test_gpu_loop_edges.py);
the scheduled variant needs 128 samples for the tile schedule's probe to run.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O

import lean_scenes as LS
import test_gpu_loop_edges as E
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

PRNGS = E.PRNGS
_ORACLE = {}


def oracle_frame(key, view, cam, p):
    """The oracle's (image, stats, rows) of p, computed once and never written to."""
    k = (key, p.width, p.height, p.samples_per_pixel, p.max_depth, p.prng, p.seed, p.sample_chunk)
    if k not in _ORACLE:
        plain = z.RenderParams(p.width, p.height, p.samples_per_pixel, p.max_depth, prng=p.prng, seed=p.seed,
                               sample_chunk=p.sample_chunk)
        img, st, rows = O.render_scanlines(view, cam, plain)
        img.setflags(write=False)
        rows.setflags(write=False)
        _ORACLE[k] = (img, st, rows)
    return _ORACLE[k]


def check_both_kernels(monkeypatch, key, view, cam, p, want_lean, schedule=None):
    """p under ZRT_LEAN=1 and ZRT_LEAN=0: the timed and the STATS flavour of each
    against the oracle (image bit for bit, Progress counters, the lockstep loop), the
    two timed frames against each other.  want_lean: the host's choice under
    ZRT_LEAN=1 (never lean under 0)."""
    ref, rs, _ = oracle_frame(key, view, cam, p)
    frames = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("ZRT_LEAN", knob)
        assert z.debug_lean_kernel(view, cam, p) == (want_lean and knob == "1"), knob
        gpu, gs = z.render(view, cam, p)
        P.assert_bit_exact(gpu, ref)
        for k in P.COUNTERS:
            assert gs[k] == rs[k], (knob, k)
        assert gs["sampling_loop"] == 3
        if schedule is not None:
            assert (gs["schedule_ms"] > 0) == schedule
        gpu2, gs2 = z.render(view, cam, dataclasses.replace(p, flags=p.flags | z.ZRT_FLAG_STATS))
        assert P.same_bits(gpu, gpu2).all(), "the STATS flavour renders other bits"
        for k in P.COUNTERS:
            assert gs2[k] == rs[k], (knob, k)
        frames[knob] = gpu
    assert P.same_bits(frames["1"], frames["0"]).all(), "the lean and the general kernel render other bits"
    return rs


def lockstep(monkeypatch):
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES", "ZRT_ATT_LDS_ROWS"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. lean against general against oracle ----------------------------------------------

@pytest.mark.parametrize("prng", list(PRNGS))
@pytest.mark.parametrize("max_depth", [1, 2, 6, 20])
@pytest.mark.parametrize("which", [2, 3])
def test_lean_general_oracle(scenes, which, max_depth, prng, monkeypatch):
    """Scenes 2 and 3 at depths 1, 2, 6, 20, both generators: the 4-sample frame with
    ZRT_FLAG_NO_SCHEDULE, and a 128-sample frame behind the tile schedule's probe (the
    probe is the general loop; the lean kernel then takes its lockstep interval and
    its tile order from it)."""
    lockstep(monkeypatch)
    s = scenes(which)
    small = dataclasses.replace(E.frame_params(max_depth, PRNGS[prng]), flags=z.ZRT_FLAG_NO_SCHEDULE)
    rs = check_both_kernels(monkeypatch, which, s.view, s.camera, small, True, schedule=False)
    assert rs["reflections"] > 0  # (paths scatter off the mesh or the ground: the shading ran)
    if max_depth >= 2:
        assert rs["rays_processed"] > rs["samples_processed"]  # (rays beyond the camera rays: rows are pushed)
    sched = E.frame_params(max_depth, PRNGS[prng], w=12, h=12, spp=128, chunk=0)  # (four tiles, partly off the frame)
    check_both_kernels(monkeypatch, which, s.view, s.camera, sched, True, schedule=True)


@pytest.mark.parametrize("rows", [0, 1])
@pytest.mark.parametrize("prng", list(PRNGS))
@pytest.mark.parametrize("which", [2, 3])
def test_lean_attenuation_rows_from_global_memory(scenes, which, prng, rows, monkeypatch):
    """Depth 20 with ZRT_ATT_LDS_ROWS 0 and 1: the lean kernel's single-class
    att_value decodes rows from global memory as well as from LDS."""
    lockstep(monkeypatch)
    monkeypatch.setenv("ZRT_ATT_LDS_ROWS", str(rows))
    s = scenes(which)
    p = E.frame_params(20, PRNGS[prng])
    plan = z.debug_launch_plan(s.view, p)
    assert plan["kmode"] == 3 and plan["att_rows"] == rows and plan["att_rows_per_path"] >= 19 - rows
    rs = check_both_kernels(monkeypatch, which, s.view, s.camera, p, True)
    # some path scatters at least three times and then reaches the sky: its product reads global rows
    deeper = oracle_frame(which, s.view, s.camera, dataclasses.replace(p, max_depth=3))[1]
    assert deeper["recursion_depth_hits"] > 0 and rs["background_hits"] > 0


# ---- 2. ineligible scenes stay general and exact --------------------------------------------

@pytest.mark.parametrize("max_depth", [1, 6])
@pytest.mark.parametrize("name", list(LS.NAMES))
def test_synthetic_scenes(name, max_depth, monkeypatch):
    """a (eligible), b (+ a dielectric sphere), c (an image texture), d (a's scene from
    outside the origin bound): the oracle's frame under both knob settings; only a is
    lean, and ZRT_LEAN=1 cannot force b-d onto the lean kernel."""
    lockstep(monkeypatch)
    _, view, cam = LS.get(name)
    p = E.frame_params(max_depth)
    rs = check_both_kernels(monkeypatch, "syn-" + name, view, cam, p, name == "a")
    assert rs["used_bvh"] == 1 and rs["reflections"] > 0
    if name == "a" and max_depth == 6:
        # b and c are not a in disguise: the glass sphere and the texels change the frame
        ref_a = oracle_frame("syn-a", view, cam, p)[0]
        for other in ("b", "c"):
            _, vo, co = LS.get(other)
            assert not P.same_bits(ref_a, oracle_frame("syn-" + other, vo, co, p)[0]).all(), other


# ---- 3. scanline rows -----------------------------------------------------------------------

@pytest.mark.parametrize("knob", ["1", "0"])
def test_scanlines_keep_the_general_kernel(scenes, knob, monkeypatch):
    """render_progress of scene 2 at depth 6: rows, image and counters are the
    oracle's under both knob settings (the flag keeps the launch off the lean kernel,
    which has no row epilogue)."""
    lockstep(monkeypatch)
    monkeypatch.setenv("ZRT_LEAN", knob)
    s = scenes(2)
    p = E.frame_params(6)
    assert not z.debug_lean_kernel(s.view, s.camera, dataclasses.replace(p, flags=z.ZRT_FLAG_SCANLINES))
    ref, rs, rrows = oracle_frame(2, s.view, s.camera, p)
    gpu, gs, rows = z.render_progress(s.view, s.camera, p)
    np.testing.assert_array_equal(rows, rrows)
    P.assert_bit_exact(gpu, ref)
    for k in P.COUNTERS:
        assert gs[k] == rs[k], k
    assert rows[:, 1].sum() == rs["reflections"] > 0


# ---- 4. two ranks ---------------------------------------------------------------------------

def test_two_ranks(scenes, monkeypatch):
    """Scene 2, 32 x 32 x 4, world_size 2: ranks 0 and 1 (lean launches of half the
    tiles each) assemble to the one-rank frame, lean and general, and to the oracle's."""
    lockstep(monkeypatch)
    s = scenes(2)
    p = z.RenderParams(32, 32, 4, 20)
    frames = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("ZRT_LEAN", knob)
        for world in (1, 2):
            for rank in range(world):
                pr = dataclasses.replace(p, rank=rank, world_size=world)
                assert z.debug_lean_kernel(s.view, s.camera, pr) == (knob == "1")
            frames[knob, world] = P.render_partitioned(s, p, world)
    one = frames["1", 1]
    for k, f in frames.items():
        assert P.same_bits(one, f).all(), k
    P.assert_bit_exact(one, oracle_frame(2, s.view, s.camera, p)[0])

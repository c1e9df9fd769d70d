"""Degenerate geometry on the GPU, bit for bit against the oracle.

The families of tests/degenerate_scenes.py through zrt_trace (every traversal, the list,
compressed nodes, the 32-bit stack on its global rows), through every sampling loop of
tests/test_gpu_loop_edges.py (image, Progress counters, scanline rows, STATS flavour),
through the lean lockstep kernel, the device BVH build and the first-hit features.  The
reference's behaviour is the specification: a leaf whose box is flat on an axis is
rejected by its loose box test (aabb.zig:109-127, tmax <= tmin) for every ray, so a grid
of triangles in an axis plane is invisible through the BVH; exact-t ties between
duplicates go to the earliest leaf in DFS order.  tests/test_degenerate_host.py asserts,
from the oracle alone, that the families do show these effects.

Finite families run first, the non-finite ones last.  The two families validate_scene
refuses (a NaN box midpoint: inf-radius, nan-center) are refusal tests on every entry
point that validates.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

import degenerate_scenes as D
import test_gpu_loop_edges as E
import test_gpu_parity as P
from test_gpu_runtime import _same_tree

pytestmark = pytest.mark.gpu

FAST, BINARY, REFERENCE = z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE
ONE = dict(width=1, height=1, samples_per_pixel=1, max_depth=1)
_REF = {}  # (name, bvh) -> the oracle's (t, prim) of the family's rays, computed once


def ref_hits(name, bvh):
    if (name, bvh) not in _REF:
        f = D.get(name)
        t, p = O.trace(f.view, bvh, f.origins, f.directions)
        t.setflags(write=False)
        p.setflags(write=False)
        _REF[name, bvh] = (t, p)
    return _REF[name, bvh]


def precondition(name):
    """The oracle-side condition that makes the family's comparison sharp (asserted in
    full by tests/test_degenerate_host.py; restated so no case here can be vacuous)."""
    f = D.get(name)
    p_list = ref_hits(name, False)[1]
    if f.n_prims <= 10:
        assert (p_list >= 0).mean() >= 0.2
        return
    p_bvh = ref_hits(name, True)[1]
    if name in D.FLAT:
        assert (p_bvh >= 0).sum() == 0 and (p_list >= 0).mean() >= 0.25
    elif name == "terraces":
        assert np.isin(p_list, f.marked).sum() - np.isin(p_bvh, f.marked).sum() >= 1000
    elif name == "duplicates":
        assert set(p_bvh[p_bvh >= 0].tolist()) != set(p_list[p_list >= 0].tolist())
    else:
        assert (p_bvh >= 0).mean() >= 0.2


def clear_knobs(monkeypatch):
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES", "ZRT_ATT_LDS_ROWS", "ZRT_STACK_LDS_ROWS",
              "ZRT_STACK_LDS_ROWS16", "ZRT_LEAN", "ZRT_BVH_DEVICE"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. closest hits -----------------------------------------------------------------------

@pytest.mark.parametrize("name", D.TRACED + ("ten",))
def test_trace(name, monkeypatch):
    """FAST, BINARY and REFERENCE against the oracle's BVH answer, the list against the
    oracle's list answer, FAST over the compressed nodes (inf-vertex: the encoder refuses
    the tree and the launch must quietly use the full nodes)."""
    clear_knobs(monkeypatch)
    precondition(name)
    f = D.get(name)
    bvh = f.n_prims > 10
    t_ref, p_ref = ref_hits(name, bvh)
    for trav in (FAST, BINARY, REFERENCE):
        t, p = z.trace(f.view, z.RenderParams(**ONE, traversal=trav), f.origins, f.directions)
        P.assert_same_hits(t, p, t_ref, p_ref)
    t_list, p_list = ref_hits(name, False)
    t, p = z.trace(f.view, z.RenderParams(**ONE, bounded_volume_hierarchy=False), f.origins, f.directions)
    P.assert_same_hits(t, p, t_list, p_list)
    monkeypatch.setenv("ZRT_QNODES", "1")
    t, p = z.trace(f.view, z.RenderParams(**ONE, traversal=FAST), f.origins, f.directions)
    P.assert_same_hits(t, p, t_ref, p_ref)


@pytest.mark.parametrize("name", ["terraces", "duplicates"])
def test_trace_replay_on_global_rows(name, monkeypatch):
    """FAST with a 32-bit stack of two LDS rows: the traversal and its reference replay
    (vertex and in-plane rays take it) run on the global rows."""
    clear_knobs(monkeypatch)
    precondition(name)
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS", "2")
    f = D.get(name)
    t_ref, p_ref = ref_hits(name, True)
    t, p = z.trace(f.view, z.RenderParams(**ONE, traversal=FAST), f.origins, f.directions)
    P.assert_same_hits(t, p, t_ref, p_ref)


# ---- 2. frames in every sampling loop --------------------------------------------------------

RENDER_CASES = [(n, l) for n in D.TRACED for l in E.BVH_LOOPS + E.LIST_LOOPS] + [("ten", l) for l in E.LIST_LOOPS]


@pytest.mark.parametrize("name,loop", RENDER_CASES, ids=[f"{n}-{l}" for n, l in RENDER_CASES])
def test_render_every_loop(name, loop, monkeypatch):
    """24 x 24, 4 spp in chunks of 3, depths 1 and 6 (terraces and duplicates: both
    generators): image, Progress counters, scanline rows and the STATS flavour against the
    oracle; the list loops with bounded_volume_hierarchy = False against the oracle's list.
    The colours are per primitive index, so the frame shows which duplicate or leaf won."""
    clear_knobs(monkeypatch)
    precondition(name)
    f = D.get(name)
    want = E.LOOPS[loop][3]
    for prng in (list(E.PRNGS) if name in ("terraces", "duplicates") else ["xoroshiro"]):
        for depth in (1, 6):
            p = E.set_edge_loop(monkeypatch, loop, E.frame_params(depth, E.PRNGS[prng]))
            if loop in E.LIST_LOOPS:
                p = dataclasses.replace(p, bounded_volume_hierarchy=False)
            plan = z.debug_launch_plan(f.view, p)
            if loop == "pool-guard":
                # nan-vertex: the guard's model of the triangles is NaN, `guard > 0` is false
                # and the flag alone asks for nothing: the lockstep loop, unguarded
                assert plan["guard_on"] == (0 if name == "nan-vertex" else 1)
                want = 5 if plan["guard_on"] else 3
            assert plan["sampling_loop"] == want, plan
            if loop == "pool-qnodes":
                assert plan["qnodes"] == (0 if name == "inf-vertex" else 1)
            gs, rs = E.check_frame(D.get, name, p)
            assert gs["sampling_loop"] == want
            assert rs["used_bvh"] == (0 if loop in E.LIST_LOOPS else 1)


def test_flat_frames_are_background_through_the_bvh():
    """What the frames above compare on the flat grids: through the BVH the oracle sees
    no triangle at all, through the list it sees the grid."""
    for name in D.FLAT:
        p = E.frame_params(6)
        assert E.oracle_frame(D.get, name, p)[1]["reflections"] == 0
        assert E.oracle_frame(D.get, name, dataclasses.replace(p, bounded_volume_hierarchy=False))[1]["reflections"] > 0


# ---- 3. the lean lockstep kernel ----------------------------------------------------------------

@pytest.mark.parametrize("name", D.LEAN)
def test_lean_kernel(name, monkeypatch):
    """Solid Lambertian / metal families seen from inside the origin bound: the lean
    kernel is the one launched (zrt_debug_lean_kernel), and ZRT_LEAN=0's general kernel
    renders the same bits: the oracle's."""
    import test_gpu_lean_kernel as LK
    clear_knobs(monkeypatch)
    precondition(name)
    f = D.get(name)
    for depth in (1, 6):
        p = E.frame_params(depth)
        monkeypatch.delenv("ZRT_LEAN", raising=False)
        assert z.debug_lean_kernel(f.view, f.camera, p)  # (the default choice, no knob set)
        LK.check_both_kernels(monkeypatch, "degenerate-" + name, f.view, f.camera, p, True)


# ---- 4. the device BVH build ----------------------------------------------------------------------

@pytest.mark.parametrize("name", D.TRACED)
def test_device_bvh_equals_host(name):
    """score_kernel's all-ties and NaN-ratio paths (a slice of total pseudo-area 0 or inf:
    the split stays n / 2 on axis 0) against the host build, node for node.  nan-vertex has
    no NaN midpoint (degenerate_scenes.py), so it builds, and equals the host tree, too."""
    f = D.get(name)
    _same_tree(z.bvh_build_device(f.view), z.bvh_build(f.view))


@pytest.mark.parametrize("name", D.REFUSED)
def test_device_bvh_refuses_nan_midpoints(name):
    f = D.get(name)
    with pytest.raises(z.ZrtError) as e:
        z.bvh_build_device(f.view)
    assert e.value.code == _ffi.ZRT_E_UNSUPPORTED


@pytest.mark.parametrize("name", ["duplicates", "inf-vertex"])
def test_render_over_the_device_built_tree(name, monkeypatch):
    clear_knobs(monkeypatch)
    precondition(name)
    f = D.get(name)
    p = E.frame_params(6)
    monkeypatch.setenv("ZRT_BVH_DEVICE", "0")
    host, hs = z.render(f.view, f.camera, p)
    monkeypatch.setenv("ZRT_BVH_DEVICE", "1")
    dev, ds = z.render(f.view, f.camera, p)
    assert P.same_bits(host, dev).all()
    for k in P.COUNTERS:
        assert hs[k] == ds[k], k
    P.assert_bit_exact(dev, E.oracle_frame(D.get, name, p)[0])


# ---- 5. first-hit features ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["terraces", "duplicates"])
def test_features(name, monkeypatch):
    """features_kernel: the surface id and the normal (and t, albedo) of each pixel's
    first hit are the oracle's, in every traversal."""
    import denoise_ref as R
    import test_gpu_denoise as DN
    clear_knobs(monkeypatch)
    precondition(name)
    f = D.get(name)
    want, _ = R.expected_features(O, f.view, f.camera, 24, 24)
    ids = np.ascontiguousarray(want[..., 7]).view(np.uint32)
    assert len(set(ids[ids > 0].tolist())) >= 2  # (primitives are seen)
    for trav in (FAST, BINARY, REFERENCE):
        got = DN.gpu_features(f.view, f.camera, z.RenderParams(24, 24, 1, 1, traversal=trav))
        DN.assert_same_bits(got[..., 7], want[..., 7], f"{name} traversal {trav}: surface id")
        DN.assert_same_bits(got[..., 0:3], want[..., 0:3], f"{name} traversal {trav}: normal")
        DN.assert_same_bits(got, want, f"{name} traversal {trav}")


# ---- 6. refused: a NaN box midpoint ---------------------------------------------------------------------

@pytest.mark.parametrize("name", D.REFUSED)
def test_nan_midpoints_are_refused(name):
    """zrt_render, zrt_render_progress, zrt_trace, zrt_ctx_create and zrt_render_multi
    refuse the scene with ZRT_E_UNSUPPORTED, naming the primitive."""
    f = D.get(name)
    p = E.frame_params(6)
    calls = [lambda: z.render(f.view, f.camera, p), lambda: z.render_progress(f.view, f.camera, p),
             lambda: z.trace(f.view, z.RenderParams(**ONE), f.origins[:64], f.directions[:64]),
             lambda: z.RenderContext(f.view, p), lambda: z.render_multi(f.view, f.camera, p, [0])]
    for call in calls:
        with pytest.raises(z.ZrtError) as e:
            call()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and f"primitive {int(f.marked[0])}:" in str(e.value), str(e.value)

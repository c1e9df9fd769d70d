"""Degenerate geometry on the host: trees, plans and the oracle-side preconditions.

The families of tests/degenerate_scenes.py (flat leaves, duplicates, zero-size and
non-finite boxes) through everything that needs no device: the host BVH build against
the oracle's node for node, the LDS / buffer / launch planners, the compressed-node
encoder and its refusal, and - from the oracle alone - the conditions that make the GPU
comparisons of tests/test_gpu_degenerate.py sharp: flat leaves really are invisible to
the reference BVH, duplicates really are won by another index than the list's, and the
rays really hit something.  A GPU test that passes is then not vacuous.
"""
import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

import degenerate_scenes as D
from test_gpu_runtime import _same_tree

_HITS = {}


def hits(name):
    """The oracle's (t, prim) of the family's rays through the BVH (None for the list
    scene) and through the list, computed once."""
    if name not in _HITS:
        f = D.get(name)
        bvh = O.trace(f.view, True, f.origins, f.directions) if f.n_prims > 10 else None
        _HITS[name] = (bvh, O.trace(f.view, False, f.origins, f.directions))
    return _HITS[name]


def test_families_are_small_and_two_coloured():
    for name in D.NAMES:
        f = D.get(name)
        assert (f.n_prims == 10) if name == "ten" else (11 <= f.n_prims <= 300), name
        assert 1000 <= len(f.origins) <= 8000 and np.isfinite(f.origins).all() and np.isfinite(f.directions).all()
        pr = D.prim_array(f.scene)
        assert len(set(pr["material"])) >= 2, name
        assert (pr["material"] == np.arange(f.n_prims) % f.n_materials).all()
    assert D.get("eleven").n_prims == 11
    # in-plane rays: o_k on the plane, d_k = 0
    for name in D.FLAT:
        f = D.get(name)
        (axis, level), = f.info["planes"]
        assert ((f.origins[:, axis] == np.float32(level)) & (f.directions[:, axis] == 0)).sum() >= 80


@pytest.mark.parametrize("name", [n for n in D.BVH_NAMES if n != "nan-center"])
def test_host_tree_equals_the_oracle(name):
    """zrt_bvh_build == oracle_bvh_build node for node: coincident centroids, boxes of
    area 0 (every SAH cost 0), overflowing centroids, +inf and NaN coordinates.
    (nan-center, where a NaN reaches the sort keys: test_refused_families_differ_or_are_unordered.)"""
    f = D.get(name)
    _same_tree(z.bvh_build(f.view), O.bvh_build(f.view))


def test_points_tree_shape():
    """The all-ties build of 32 primitives at one point (plus two ordinary ones)."""
    f = D.get("points")
    mins, maxs, left, _, depth = z.bvh_build(f.view)
    assert len(D.flat_leaves(mins, maxs, left)) >= 15 and depth >= 5


def test_refused_families_differ_or_are_unordered():
    """Why validate_scene refuses a NaN midpoint: `<` does not order it, so the tree is
    the sort algorithm's, not the scene's.  nan-center: the host build's std::stable_sort
    and the oracle's merge sort (each the reference's stable sort on ordered keys) give
    different trees.  inf-radius: they happen to agree (kept: test_host_tree_equals_the_oracle)."""
    f = D.get("nan-center")
    h, o = z.bvh_build(f.view), O.bvh_build(f.view)
    assert len(h[2]) == len(o[2]) and not ((h[2] == o[2]).all() and (h[3] == o[3]).all())
    for name in D.REFUSED:
        pr = D.prim_array(D.get(name).scene)
        lo, hi = pr["center"] - pr["radius"][:, None], pr["center"] + pr["radius"][:, None]
        with np.errstate(invalid="ignore"):
            assert np.isnan((lo + hi) / np.float32(2)).any(1).sum() == 1


@pytest.mark.parametrize("name", D.REFUSED)
def test_nan_midpoints_are_refused_up_front(name):
    """Every entry point that validates and needs no device names the primitive."""
    f = D.get(name)
    p = z.RenderParams(24, 24, 4, 6, sample_chunk=3)
    calls = [lambda: z.debug_lds_plans(f.view), lambda: z.debug_buffer_plans(f.view), lambda: z.debug_qnodes(f.view),
             lambda: z.debug_launch_plan(f.view, p), lambda: z.debug_lean_kernel(f.view, f.camera, p)]
    for call in calls:
        with pytest.raises(z.ZrtError) as e:
            call()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and f"primitive {int(f.marked[0])}:" in str(e.value), str(e.value)


def test_nothing_finite_is_refused():
    for name in D.FINITE + ("inf-vertex", "nan-vertex"):
        assert z.debug_lds_plans(D.get(name).view) > 0


@pytest.mark.parametrize("name", [n for n in D.NAMES if n not in D.REFUSED])
def test_plans_succeed(name):
    f = D.get(name)
    assert z.debug_lds_plans(f.view) > 0
    assert z.debug_buffer_plans(f.view) > (0 if f.n_prims > 10 else -1)  # (a list scene has no such rows: succeeds with 0)
    plan = z.debug_launch_plan(f.view, z.RenderParams(24, 24, 4, 6, sample_chunk=3))
    if name == "ten":
        assert plan["sampling_loop"] in (0, 6), plan  # a list loop
    else:
        assert plan["sampling_loop"] == 3, plan


@pytest.mark.parametrize("name", D.TRACED)
def test_qnodes_encode_or_refuse(name, monkeypatch):
    """The compressed-node encoder checks every finite family's tree and refuses the
    inf-vertex tree (quantize_wide ok = false: "a non-finite plane"); a launch that asks
    for compressed nodes (ZRT_QNODES=1, ZRT_POOL=1) then plans the full ones, qnodes == 0.
    (inf-radius raises ZRT_E_UNSUPPORTED too, one step earlier:
    test_nan_midpoints_are_refused_up_front.)

    nan-vertex encodes: the reference's box of a triangle (triangle.zig:33, min / max of
    the vertices) drops a NaN operand, so the triangle ((0,0,-1), (NaN,0,-1), (0,1,-1))
    gets the finite flat box x in [0, 0] and no NaN reaches the tree."""
    f = D.get(name)
    refused = name == "inf-vertex"
    if refused:
        with pytest.raises(z.ZrtError) as e:
            z.debug_qnodes(f.view)
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and "refused" in str(e.value)
    else:
        assert z.debug_qnodes(f.view) > 0
    if name == "nan-vertex":
        mins, maxs, _, _, _ = O.bvh_build(f.view)
        assert np.isfinite(mins).all() and np.isfinite(maxs).all()
    monkeypatch.setenv("ZRT_QNODES", "1")
    monkeypatch.setenv("ZRT_POOL", "1")
    monkeypatch.setenv("ZRT_WF", "0")
    plan = z.debug_launch_plan(f.view, z.RenderParams(24, 24, 4, 6, sample_chunk=3))
    assert plan["sampling_loop"] == 5
    assert plan["qnodes"] == (0 if refused else 1), plan


# ---- the oracle-side preconditions of the GPU comparisons -------------------------------

@pytest.mark.parametrize("name", D.FLAT)
def test_flat_grid_is_invisible_to_the_reference_bvh(name):
    f = D.get(name)
    (_, p_bvh), (_, p_list) = hits(name)
    assert (p_bvh >= 0).sum() == 0
    assert (p_list >= 0).sum() >= 0.25 * len(f.origins)
    mins, maxs, left, _, _ = O.bvh_build(f.view)
    assert len(D.flat_leaves(mins, maxs, left)) == (left < 0).sum() and (mins[0] == maxs[0]).any()


def test_terraces_hide_their_flat_leaves():
    f = D.get("terraces")
    mins, maxs, left, _, _ = O.bvh_build(f.view)
    assert len(D.flat_leaves(mins, maxs, left)) >= 20
    assert len(D.flat_leaves(mins, maxs, left)) < (left < 0).sum()  # (a thick tree: not every leaf)
    (_, p_bvh), (_, p_list) = hits("terraces")
    on_flat_bvh, on_flat_list = np.isin(p_bvh, f.marked).sum(), np.isin(p_list, f.marked).sum()
    assert on_flat_bvh > 0  # (leaves pairing two terraces are thick: some flat triangles are seen)
    assert on_flat_list - on_flat_bvh >= 1000


def test_duplicates_are_won_by_dfs_order():
    (_, p_bvh), (_, p_list) = hits("duplicates")
    w_bvh, w_list = set(p_bvh[p_bvh >= 0].tolist()), set(p_list[p_list >= 0].tolist())
    assert w_bvh != w_list, (w_bvh, w_list)
    assert len(w_bvh) == 2 and len(w_list) == 2  # one sphere and one triangle each
    # the two winners of a kind differ in material: a render shows which one won
    f = D.get("duplicates")
    pr = D.prim_array(f.scene)
    s_bvh, s_list = min(w_bvh), min(w_list)
    assert pr["kind"][s_bvh] == pr["kind"][s_list] == 0 and pr["material"][s_bvh] != pr["material"][s_list]
    # ... and so do the first (the winner) and the last duplicate of each kind in DFS order
    _, _, left, right, _ = O.bvh_build(f.view)
    dfs = []
    for i in np.nonzero(left < 0)[0]:
        for c in (left[i], right[i]):
            if -c - 1 not in dfs:
                dfs.append(int(-c - 1))
    for kind in (0, 1):
        k = [p for p in dfs if pr["kind"][p] == kind]
        assert k[0] in w_bvh and pr["material"][k[0]] != pr["material"][k[-1]], (k[0], k[-1])


@pytest.mark.parametrize("name", ["points", "slivers", "range", "eleven"])
def test_rays_hit_something(name):
    f = D.get(name)
    (_, p_bvh), _ = hits(name)
    assert (p_bvh >= 0).sum() >= 0.2 * len(f.origins)
    if name == "slivers":
        for (_, p) in hits(name):
            assert not np.isin(p, f.marked).any()
    if name == "points":  # (a radius-0 sphere is hit by rays through its centre; a point triangle never)
        pr = D.prim_array(f.scene)
        assert not (pr["kind"][p_bvh[p_bvh >= 0]] == 1)[np.isin(p_bvh[p_bvh >= 0], f.marked)].any()


def test_ten_is_the_eleven_minus_one():
    a, b = D.prim_array(D.get("ten").scene), D.prim_array(D.get("eleven").scene)
    assert a.tobytes() == b[:10].tobytes()

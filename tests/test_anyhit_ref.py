"""The any-hit reference of tests/anyhit_ref.py, pinned on the CPU (no kernel launches):

* the literal restatement of bvh.zig:187-205 started at t_max = +inf is oracle_trace,
  in hit / miss and in t;
* the per-leaf form equals the literal one at every t_max of t_max_sets;
* the ray sets stay adversarial: the counts below are half of what was measured when the
  feature was written (DESIGN.md §5 "Ray queries"), so a generator that drifts towards
  easy rays fails here and not silently in tests/test_gpu_queries.py;
* the new entry points are exported and bound, and refuse what they can without a device.
"""
import ctypes as C

import numpy as np
import pytest

import adversarial_rays as A
import anyhit_ref as R
import degenerate_scenes as D
import hazard_rays as H
import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

F = np.float32


class Case(R.RayCase):
    """n_literal: the leading rays the (slow) literal form is run on."""

    def __init__(self, scene, o, d, n_literal=None):
        super().__init__(O, scene, o, d)
        self.n_literal = len(o) if n_literal is None else n_literal

    def head(self):
        k = self.n_literal
        return self.o[:k], self.d[:k]


@pytest.fixture(scope="module")
def hazard():
    return Case(*H.hazard_scene(seed=1, n_rays=3000))


@pytest.fixture(scope="module")
def near_miss():
    return Case(*A.near_miss_scene(seed=0, n_rays=4000), n_literal=600)


@pytest.fixture(scope="module")
def terraces():
    f = D.get("terraces")
    mins, maxs, left, _, _ = O.bvh_build(f.view)
    assert len(D.flat_leaves(mins, maxs, left)) > 0  # the family with flat leaves inside a thick tree
    return Case(f.scene, f.origins[::4], f.directions[::4])


CASES = ["hazard", "near_miss", "terraces"]


@pytest.mark.parametrize("name", CASES)
def test_literal_at_infinity_is_oracle_trace(name, request):
    c = request.getfixturevalue(name)
    o, d = c.head()
    t = R.literal_t(O, c.view, c.nodes, o, d)
    k = len(o)
    assert np.array_equal(np.isfinite(t), c.p_ref[:k] >= 0)
    assert np.array_equal(t.view(np.uint32), c.t_ref[:k].view(np.uint32))


@pytest.mark.parametrize("name", CASES)
def test_leafwise_equals_literal(name, request):
    c = request.getfixturevalue(name)
    o, d = c.head()
    k = len(o)
    for key in (None,) + R.SETS:
        tm = None if key is None else c.sets[key][:k]
        lit = R.literal(O, c.view, c.nodes, o, d, tm)
        leaf = R.leafwise(O, c.view, c.nodes, o, d, tm)
        assert np.array_equal(lit, leaf), (name, key, int((lit != leaf).sum()))


def test_hazard_set_stays_adversarial(hazard):
    c = hazard
    # strictness: nothing is occluded at the reference's own closest t, although half the
    # rays have a primitive hit below it (the list's answer)
    occ = R.leafwise(O, c.view, c.nodes, c.o, c.d, c.sets["t_ref"])
    assert occ.sum() == 0
    assert (c.t_list < c.sets["t_ref"]).sum() >= 750
    # one ulp above it the closest hit's own leaf still fails the loose test on many rays
    occ = R.leafwise(O, c.view, c.nodes, c.o, c.d, c.sets["next(t_ref)"])
    assert (~occ).sum() >= 170


def test_near_miss_set_stays_adversarial(near_miss):
    c = near_miss
    hit = c.p_ref >= 0
    assert hit.sum() >= 1200
    occ = R.leafwise(O, c.view, c.nodes, c.o, c.d, c.sets["2 t_ref"])
    assert (hit & ~occ).sum() >= 29  # hit at +inf, not occluded at twice that t: a finite t_max clips the slabs
    tm = (np.where(hit, c.t_ref, F(1.0)) * F(1 + 2.0 ** -8)).astype(F)
    occ = R.leafwise(O, c.view, c.nodes, c.o, c.d, tm)
    assert (hit & ~occ).sum() >= 55


def test_list_form_is_strict():
    f = D.get("ten")
    o, d = f.origins[:300], f.directions[:300]
    t_list, p = O.trace(f.view, False, o, d)
    assert (p >= 0).sum() > 50
    tm = np.where(np.isfinite(t_list), t_list, F(1.0)).astype(F)
    assert not R.literal_list(O, f.view, o, d, tm).any()
    assert np.array_equal(R.literal_list(O, f.view, o, d, np.nextafter(tm, F(np.inf))), p >= 0)
    assert np.array_equal(R.literal_list(O, f.view, o, d), p >= 0)


def test_query_symbols_exported_and_bound():
    lib = _ffi.load()
    assert lib.zrt_abi_version() == 2 == _ffi.ABI_VERSION
    names = {n for n, _, _ in _ffi.SIGNATURES}
    for name in ("zrt_ctx_trace", "zrt_ctx_occluded", "zrt_occluded", "zrt_ctx_query_ms"):
        assert name in names and hasattr(lib, name), name
    for attr in ("trace", "occluded", "query_ms"):
        assert callable(getattr(z.RenderContext, attr))
    assert callable(z.occluded)


def test_query_refusals_without_a_device():
    lib = _ffi.load()
    p = z.RenderParams(1, 1, 1, 1).abi()
    ms = C.c_double()
    buf = (C.c_float * 6)()
    out = (C.c_uint8 * 1)()
    # a null context, null params
    assert lib.zrt_ctx_trace(None, C.byref(p), None, 0, None, None, None) == _ffi.ZRT_E_INVALID
    assert lib.zrt_ctx_occluded(None, C.byref(p), None, None, 0, None, None) == _ffi.ZRT_E_INVALID
    assert lib.zrt_ctx_query_ms(None, C.byref(ms)) == _ffi.ZRT_E_INVALID
    f = D.get("eleven")
    assert lib.zrt_occluded(f.view, None, buf, None, 1, out) == _ffi.ZRT_E_INVALID
    # null rays / output with n > 0, an unknown traversal: refused before any device is looked for
    assert lib.zrt_occluded(f.view, C.byref(p), None, None, 1, out) == _ffi.ZRT_E_INVALID
    assert lib.zrt_occluded(f.view, C.byref(p), buf, None, 1, None) == _ffi.ZRT_E_INVALID
    p.traversal = 3
    assert lib.zrt_occluded(f.view, C.byref(p), buf, None, 1, out) == _ffi.ZRT_E_INVALID
    assert b"traversal" in lib.zrt_last_error()
    # a scene validate_scene refuses is refused here too
    p.traversal = 0
    assert lib.zrt_occluded(D.get("nan-center").view, C.byref(p), buf, None, 1, out) == _ffi.ZRT_E_UNSUPPORTED

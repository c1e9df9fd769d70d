"""GPU tests of the ray queries on a resident context (zrt.h "ray queries"):

1. zrt_ctx_trace equals zrt_trace and oracle_trace bit for bit, at wave and block edges,
   twice on one context, on a torch stream, and leaves a later render exact;
2. any-hit at t_max = +inf is oracle_trace's hit / miss on every adversarial set;
3. any-hit at finite t_max is tests/anyhit_ref.py's answer (the definition: what
   rayColor's surface loop returns when started with t_max) for every set of
   t_max_sets - a "closest hit below t_max" or "any primitive below t_max" rule fails
   here on hundreds of rays (tests/test_anyhit_ref.py pins how many);
4. the same through the stack's global overflow rows;
5. the device error convention; 6. the one-shot zrt_occluded.
"""
import functools

import numpy as np
import pytest

import adversarial_rays as A
import anyhit_ref as R
import degenerate_scenes as D
import grazing_rays as G
import grazing_tris as GT
import hazard_rays as H
import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

pytestmark = pytest.mark.gpu
F = np.float32
TRAVERSALS = [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE]
TRAV_IDS = ["fast", "binary", "reference"]
FILL_T, FILL_P, FILL_B = -7.5, -77, 7  # what over-allocated outputs hold past n


def params(trav=z.ZRT_TRAVERSAL_FAST, bvh=True):
    return z.RenderParams(1, 1, 1, 1, bounded_volume_hierarchy=bvh, traversal=trav)


def rays_of(o, d):
    return np.ascontiguousarray(np.concatenate([np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)], 1))


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ctx_trace(ctx, p, rays_dev, n, stream=0):
    """(t, prim) of the first n rays; the outputs are 64 elements longer and keep their fill there."""
    import torch
    t = torch.full((n + 64,), FILL_T, dtype=torch.float32, device="cuda")
    prim = torch.full((n + 64,), FILL_P, dtype=torch.int32, device="cuda")
    if stream:
        torch.cuda.synchronize()  # (the fills ran on torch's current stream)
    ctx.trace(p, rays_dev.data_ptr(), n, t.data_ptr(), prim.data_ptr(), stream)
    ctx.sync()
    torch.cuda.synchronize()
    th, ph = t.cpu().numpy(), prim.cpu().numpy()
    assert (th[n:] == F(FILL_T)).all() and (ph[n:] == FILL_P).all(), "a query wrote past n"
    return th[:n], ph[:n]


def ctx_occluded(ctx, p, rays_dev, n, t_max=None, stream=0):
    import torch
    out = torch.full((n + 64,), FILL_B, dtype=torch.uint8, device="cuda")
    tm = to_dev(np.ascontiguousarray(t_max, F)) if t_max is not None else None
    if stream:
        torch.cuda.synchronize()
    ctx.occluded(p, rays_dev.data_ptr(), tm.data_ptr() if tm is not None else 0, n, out.data_ptr(), stream)
    ctx.sync()
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert (h[n:] == FILL_B).all(), "a query wrote past n"
    assert np.isin(h[:n], (0, 1)).all()
    return h[:n] != 0


def assert_same_hits(t, p, t_ref, p_ref, what=""):
    bad = (p != p_ref) | (t.view(np.uint32) != t_ref.view(np.uint32))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {len(t)} rays differ, first {int(np.argmax(bad))}"


def assert_equal(got, want, what=""):
    bad = got != want
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {len(got)} rays differ (got occluded, want not: "
                           f"{int((got & ~want).sum())}), first {int(np.argmax(bad))}")


def random_rays(scene, n, seed):
    """Rays from a shell around the scene's small primitives at points among them."""
    pr = R.prim_array(scene)
    tri, sph = pr[pr["kind"] == 1], pr[(pr["kind"] == 0) & (pr["radius"] < 50)]
    pts = np.concatenate([tri["a"], tri["b"], tri["c"], sph["center"]]).astype(np.float64)
    lo, hi = pts.min(0), pts.max(0)
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(lo, hi, (n, 3))
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (tgt + v * float(np.max(hi - lo)) * rng.uniform(0.8, 2.0, (n, 1))).astype(F)
    return o, (tgt - o).astype(F)


# ---- the cases: scenes, rays and references, built once --------------------------------

@functools.lru_cache(maxsize=None)
def hazard_case():
    return R.RayCase(O, *H.hazard_scene(seed=1, n_rays=3000))


@functools.lru_cache(maxsize=None)
def near_miss_case():
    return R.RayCase(O, *A.near_miss_scene(seed=0, n_rays=4000))


_MESH = {}


def mesh_case(scenes, which):
    """Scene 2 / 3 with the grazing rays and the grazing-triangle rays of the parity tests."""
    if which not in _MESH:
        s = scenes(which)
        pr = R.prim_array(s)
        mins, maxs, left, right, _ = O.bvh_build(s.view)
        o1, d1 = G.grazing_rays(pr, mins, maxs, left, n=6000, seed=7, span=float(np.max(maxs[0] - mins[0])))
        o2, d2 = GT.grazing_triangle_rays(pr, mins, maxs, left, right, n=20000, seed=1, span=GT.scene_span(pr))
        c = R.RayCase(O, s, np.concatenate([o1, o2]), np.concatenate([d1, d2]), keep=s)
        # the literal form's subsample: 100 rays of each generator
        c.sub = np.concatenate([np.linspace(0, len(o1) - 1, 100).astype(np.int64),
                                len(o1) + np.linspace(0, len(o2) - 1, 100).astype(np.int64)])
        _MESH[which] = c
    return _MESH[which]


class Resident:
    """A context on a case's scene with the case's rays on the device."""

    def __init__(self, case, bvh=True):
        self.case = case
        self.ctx = z.RenderContext(case.view, params(bvh=bvh))
        self.rays = to_dev(rays_of(case.o, case.d))
        self.n = len(case.o)

    def occluded(self, trav, t_max=None, bvh=True):
        return ctx_occluded(self.ctx, params(trav, bvh), self.rays, self.n, t_max)

    def close(self):
        self.ctx.close()


# ---- 1. the resident closest hit --------------------------------------------------------

def _trace_scene(scenes, name):
    if name == "hazard":
        c = hazard_case()
        return c.view, None, c.o, c.d
    s = scenes(name)
    o, d = random_rays(s, 3000, seed=name)
    return s.view, s, o, d


@pytest.mark.parametrize("name", [1, 2, "hazard"], ids=["scene1-list", "scene2", "hazard"])
def test_ctx_trace_equals_trace_and_oracle(scenes, name):
    import torch
    view, keep, o, d = _trace_scene(scenes, name)
    use_bvh = view.contents.n_prims > 10
    assert use_bvh == (name != 1)
    t_ref, p_ref = O.trace(view, use_bvh, o, d)
    assert (p_ref >= 0).mean() > 0.2 and (name == "hazard" or (p_ref < 0).any())
    rays = to_dev(rays_of(o, d))
    for trav in TRAVERSALS if use_bvh else TRAVERSALS[:1]:
        p = params(trav)
        t1, p1 = z.trace(view, p, o, d)
        assert_same_hits(t1, p1, t_ref, p_ref, "zrt_trace")
        ctx = z.RenderContext(view, p)
        try:
            for n in (1, 63, 64, 65, 255, 256, 257, 3000):
                t, pr = ctx_trace(ctx, p, rays, n)
                assert_same_hits(t, pr, t_ref[:n], p_ref[:n], f"traversal {trav}, n = {n}")
            # a second batch of other rays on the same context, and on a torch stream
            rays2 = to_dev(rays_of(o[::-1], d[::-1]))
            t, pr = ctx_trace(ctx, p, rays2, 3000)
            assert_same_hits(t, pr, t_ref[::-1], p_ref[::-1], "second batch")
            st = torch.cuda.Stream()
            t, pr = ctx_trace(ctx, p, rays, 257, stream=st.cuda_stream)
            assert_same_hits(t, pr, t_ref[:257], p_ref[:257], "torch stream")
            assert ctx.query_ms() > 0.0
            # n == 0: ZRT_OK, nothing enqueued, null pointers allowed
            ctx.trace(p, 0, 0, 0, 0)
            ctx.occluded(p, 0, 0, 0, 0)
            # the context still renders the oracle's frame
            if keep is not None:
                rp = z.RenderParams(16, 16, 2, 8, traversal=trav)
                tiles = torch.zeros(ctx.tile_count(rp) * 64 * 3, dtype=torch.float32, device="cuda")
                frame = torch.zeros(16 * 16 * 3, dtype=torch.float32, device="cuda")
                ctx.render_tiles(keep.camera, rp, tiles.data_ptr())
                ctx.assemble(rp, tiles.data_ptr(), frame.data_ptr())
                ctx.sync()
                torch.cuda.synchronize()
                ref, rst = O.render(view, keep.camera, rp)
                img = frame.cpu().numpy().reshape(16, 16, 3)
                assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
                assert ctx.stats()["rays_processed"] == rst["rays_processed"]
                # ... and a query between two renders leaves the next one exact too
                t, pr = ctx_trace(ctx, p, rays, 65)
                assert_same_hits(t, pr, t_ref[:65], p_ref[:65], "after a render")
        finally:
            ctx.close()


def test_query_argument_refusals(scenes):
    import torch
    s = scenes(2)
    p = params()
    ctx = z.RenderContext(s, p)
    buf = torch.zeros(64, dtype=torch.float32, device="cuda")
    ptr = buf.data_ptr()
    try:
        for call in (lambda: ctx.trace(p, 0, 4, ptr, ptr), lambda: ctx.trace(p, ptr, 4, 0, ptr),
                     lambda: ctx.trace(p, ptr, 4, ptr, 0), lambda: ctx.trace(p, ptr + 2, 4, ptr, ptr),
                     lambda: ctx.occluded(p, 0, 0, 4, ptr), lambda: ctx.occluded(p, ptr, 0, 4, 0),
                     lambda: ctx.occluded(p, ptr, ptr + 1, 4, ptr),
                     lambda: ctx.occluded(params(bvh=False), ptr, 0, 4, ptr),   # another BVH decision
                     lambda: ctx.occluded(params(trav=3), ptr, 0, 4, ptr)):
            with pytest.raises(z.ZrtError) as e:
                call()
            assert e.value.code == _ffi.ZRT_E_INVALID
    finally:
        ctx.close()


# ---- 2. any-hit at t_max = +inf -----------------------------------------------------------

def _inf_check(view, o, d, use_bvh, what):
    _, p_ref = O.trace(view, use_bvh, o, d)
    want = p_ref >= 0
    n = len(o)
    rays = to_dev(rays_of(o, d))
    ctx = z.RenderContext(view, params(bvh=use_bvh))
    try:
        for trav in TRAVERSALS if use_bvh else TRAVERSALS[:1]:
            p = params(trav, use_bvh)
            assert_equal(ctx_occluded(ctx, p, rays, n), want, f"{what}, traversal {trav}, NULL t_max")
            assert_equal(ctx_occluded(ctx, p, rays, n, np.full(n, np.inf, F)), want, f"{what}, traversal {trav}, +inf")
    finally:
        ctx.close()
    return want


def test_anyhit_at_infinity_hazard_and_near_miss():
    for c, what in ((hazard_case(), "hazard"), (near_miss_case(), "near-miss")):
        want = _inf_check(c.view, c.o, c.d, True, what)
        assert np.array_equal(want, c.expected(None))  # (the reference agrees with oracle_trace there)


@pytest.mark.parametrize("which", [2, 3])
def test_anyhit_at_infinity_grazing(scenes, which):
    c = mesh_case(scenes, which)
    want = _inf_check(c.view, c.o, c.d, True, f"scene {which}")
    assert 0.5 < want.mean() < 1.0


@pytest.mark.parametrize("name", D.TRACED + ("ten",))
def test_anyhit_at_infinity_degenerate(name):
    f = D.get(name)
    _inf_check(f.view, f.origins, f.directions, f.n_prims > 10, name)


def test_anyhit_at_infinity_scene1_without_bvh(scenes):
    s = scenes(1)
    o, d = random_rays(s, 3000, seed=5)
    want = _inf_check(s.view, o, d, False, "scene 1")
    assert 0.2 < want.mean() < 1.0


# ---- 3. any-hit at finite t_max -----------------------------------------------------------

@pytest.mark.parametrize("case", [hazard_case, near_miss_case], ids=["hazard", "near-miss"])
def test_anyhit_finite_equals_the_reference(case):
    c = case()
    r = Resident(c)
    try:
        for key in R.SETS:
            want = c.expected(key)
            for trav in TRAVERSALS:
                assert_equal(r.occluded(trav, c.sets[key]), want, f"set {key}, traversal {trav}")
        # strictness: where the list's closest hit is the BVH's, nothing lies below t_ref
        only = np.isfinite(c.t_ref) & (c.t_list == c.t_ref)
        for trav in TRAVERSALS:
            assert not r.occluded(trav, c.sets["t_ref"])[only].any()
        # NaN, 0, 0.001 and negative t_max: nothing
        for v in (np.nan, 0.0, 0.001, -1.0, -np.inf):
            for trav in TRAVERSALS:
                assert not r.occluded(trav, np.full(len(c), v, F)).any(), (v, trav)
    finally:
        r.close()


@pytest.mark.parametrize("which", [2, 3])
def test_anyhit_finite_on_meshes(scenes, which):
    """REFERENCE against the literal form on a 200-ray subsample; FAST and BINARY against
    REFERENCE on the full grazing sets."""
    c = mesh_case(scenes, which)
    r = Resident(c)
    try:
        so, sd = c.o[c.sub], c.d[c.sub]
        only = np.isfinite(c.t_ref) & (c.t_list == c.t_ref)
        assert only.sum() > 1000
        for key in R.SETS:
            ref = r.occluded(z.ZRT_TRAVERSAL_REFERENCE, c.sets[key])
            lit = R.literal(O, c.view, c.nodes, so, sd, c.sets[key][c.sub])
            assert_equal(ref[c.sub], lit, f"scene {which}, set {key}, REFERENCE against the literal form")
            for trav in (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY):
                assert_equal(r.occluded(trav, c.sets[key]), ref, f"scene {which}, set {key}, traversal {trav}")
            if key == "t_ref":
                assert not ref[only].any()
        for v in (np.nan, 0.0, 0.001, -1.0):
            for trav in TRAVERSALS:
                assert not r.occluded(trav, np.full(len(c), v, F)).any(), (v, trav)
    finally:
        r.close()


def test_anyhit_finite_list_path():
    """The surface list (ten primitives): the strict tests against the fixed t_max."""
    f = D.get("ten")
    o, d = f.origins, f.directions
    t_list, pl = O.trace(f.view, False, o, d)
    tm = np.where(np.isfinite(t_list), t_list, F(1.0)).astype(F)
    rays = to_dev(rays_of(o, d))
    ctx = z.RenderContext(f.view, params())
    try:
        for t_max in (tm, np.nextafter(tm, F(np.inf)), (tm * F(0.5)).astype(F), (tm * F(2)).astype(F)):
            want = R.literal_list(O, f.view, o, d, t_max)
            assert_equal(ctx_occluded(ctx, params(), rays, len(o), t_max), want, "list path")
        assert not ctx_occluded(ctx, params(), rays, len(o), tm).any()
    finally:
        ctx.close()


# ---- 4. the stack's overflow rows --------------------------------------------------------

@pytest.mark.parametrize("hook", ["ZRT_STACK_LDS_ROWS", "ZRT_STACK_LDS_ROWS16"])
def test_anyhit_overflow_rows(scenes, hook, monkeypatch):
    monkeypatch.setenv(hook, "2")
    c = hazard_case()
    r = Resident(c)
    try:
        for key in R.SETS:
            for trav in TRAVERSALS:
                assert_equal(r.occluded(trav, c.sets[key]), c.expected(key), f"{hook}, set {key}, traversal {trav}")
    finally:
        r.close()
    # a deep tree, whose pushes really reach the global rows
    m = mesh_case(scenes, 2)
    k = 8000
    rays = to_dev(rays_of(m.o[:k], m.d[:k]))
    ctx = z.RenderContext(m.view, params())
    try:
        got = ctx_occluded(ctx, params(), rays, k, m.sets["2 t_ref"][:k])
        t, pr = ctx_trace(ctx, params(), rays, k)
    finally:
        ctx.close()
    monkeypatch.delenv(hook)
    ctx = z.RenderContext(m.view, params())
    try:
        assert_equal(got, ctx_occluded(ctx, params(), rays, k, m.sets["2 t_ref"][:k]), hook)
    finally:
        ctx.close()
    assert_same_hits(t, pr, m.t_ref[:k], m.p_ref[:k], hook)


# ---- 5. the device error convention ------------------------------------------------------

@pytest.mark.parametrize("trav", TRAVERSALS, ids=TRAV_IDS)
def test_query_stack_overflow_is_reported(scenes, trav, monkeypatch):
    """A stack too small for the tree (ZRT_DEBUG_STACK_CAP) sets the query's error flag:
    zrt_ctx_sync reports ZRT_E_UNSUPPORTED once, the outputs hold NaN / -1 / 0xFF, and the
    context answers correctly afterwards."""
    import torch
    s = scenes(2)
    o, d = random_rays(s, 1000, seed=3)
    _, p_ref = O.trace(s.view, True, o, d)
    rays = to_dev(rays_of(o, d))
    n = len(o)
    p = params(trav)
    ctx = z.RenderContext(s, p)
    t = torch.zeros(n, dtype=torch.float32, device="cuda")
    prim = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    try:
        monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
        ctx.trace(p, rays.data_ptr(), n, t.data_ptr(), prim.data_ptr())
        with pytest.raises(z.ZrtError) as e:
            ctx.sync()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and "overflow" in str(e.value)
        assert torch.isnan(t).all() and (prim == -1).all()
        ctx.sync()  # reported once
        ctx.occluded(p, rays.data_ptr(), 0, n, out.data_ptr())
        with pytest.raises(z.ZrtError) as e:
            ctx.sync()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED
        assert (out == 0xFF).all()
        with pytest.raises(z.ZrtError) as e:
            z.occluded(s, p, o, d)
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED
        monkeypatch.delenv("ZRT_DEBUG_STACK_CAP")
        assert_equal(ctx_occluded(ctx, p, rays, n), p_ref >= 0, "after the error")
    finally:
        ctx.close()


# ---- 6. the one-shot entry point ---------------------------------------------------------

def test_one_shot_occluded_equals_the_context_path(scenes):
    c = hazard_case()
    for trav in TRAVERSALS:
        for key in (None, "next(t_ref)", "2 t_ref"):
            got = z.occluded(c.view, params(trav), c.o, c.d, c.t_max(key))
            assert_equal(got, c.expected(key), f"one-shot, set {key}, traversal {trav}")
    s = scenes(1)
    o, d = random_rays(s, 500, seed=9)
    t_list, pl = O.trace(s.view, False, o, d)
    assert np.array_equal(z.occluded(s, params(), o, d), pl >= 0)
    tm = np.where(np.isfinite(t_list), t_list, F(1.0)).astype(F)
    assert not z.occluded(s, params(), o, d, tm).any()
    assert np.array_equal(z.occluded(s, params(), o, d, np.nextafter(tm, F(np.inf))), pl >= 0)

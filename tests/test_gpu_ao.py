"""GPU tests of the ambient-occlusion plane (zrt.h "ambient occlusion"; zrt_ctx_ao):

1. counts equal tests/ao_ref.py's composition on the shading scenes, every traversal, both
   PRNGs, the radius +inf and finite; ao is bit-equal to float(c) / float(n).  The features
   are the oracle-composed buffer, uploaded: ao_kernel is tested apart from features_kernel;
2. the loaded scenes: the surface list (scene 1) and the bunny (scene 2);
3. shape edges: sample counts on both reductions, ragged groups and tiles, columns outside D;
4. accumulation; 5. consistency with zrt_ctx_occluded on the GPU's own feature buffer;
6. synthetic features (poisoned pixels, misses with garbage); 7. refusals; 8. the device
error convention; 9. no interference with a run, a render or a stream; 10. the one-shot
call and the CLI.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import ao_ref as AO
import shading_scenes as S
import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

pytestmark = pytest.mark.gpu
F = np.float32
TRAVERSALS = [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE]
FILL_C, FILL_A = 0x7A7A7A7A, -7.5  # what over-allocated outputs hold past width * height
ACC = _ffi.ZRT_AO_ACCUMULATE
_KEEP = {}


def scene_of(key, scenes):
    """key: a name of shading_scenes.NAMES or a loaded scene's index -> (view, camera)."""
    if isinstance(key, int):
        s = scenes(key)
        return s.view, s.camera
    _, view, cam = S.get(key)
    return view, cam


def ref_case(scenes, key, w, h, radius=math.inf, prng=0, seed=42):
    """The reference of one (scene, frame, radius, PRNG), built once and kept."""
    k = (key, w, h, float(radius), prng, seed)
    if k not in _KEEP:
        view, cam = scene_of(key, scenes)
        feat = _KEEP.get(("features", key, w, h))
        c = AO.AoCase(O, view, cam, w, h, radius=radius, seed=seed, prng=prng, features=feat)
        _KEEP[("features", key, w, h)] = c.features
        _KEEP[k] = c
    return _KEEP[k]


def params(w, h, trav=z.ZRT_TRAVERSAL_FAST, prng=0, seed=42, **kw):
    return z.RenderParams(w, h, 1, 1, traversal=trav, prng=prng, seed=seed, **kw)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_ao(ctx, cam, p, ao, feat_dev, prior=None, want_ao=True, stream=0, sync=True):
    """One zrt_ctx_ao: (clear uint32[h, w], ao float32[h, w] or None).  The outputs are 64
    elements longer and must keep their fill there; prior: what dev_clear holds before."""
    import torch
    n = p.width * p.height
    clear = torch.full((n + 64,), FILL_C, dtype=torch.int32, device="cuda")
    if prior is not None:
        clear[:n] = to_dev(np.ascontiguousarray(prior, np.uint32).view(np.int32).ravel())
    plane = torch.full((n + 64,), FILL_A, dtype=torch.float32, device="cuda") if want_ao else None
    torch.cuda.synchronize()  # (the fills ran on torch's current stream)
    ctx.ao(cam, p, ao, feat_dev.data_ptr(), clear.data_ptr(), plane.data_ptr() if want_ao else 0, stream)
    if sync:
        ctx.sync()
    torch.cuda.synchronize()
    c = clear.cpu().numpy().view(np.uint32)
    assert (c[n:] == FILL_C).all(), "zrt_ctx_ao wrote past the count plane"
    a = None
    if want_ao:
        a = plane.cpu().numpy()
        assert (a[n:] == F(FILL_A)).all(), "zrt_ctx_ao wrote past the ao plane"
        a = a[:n].reshape(p.height, p.width)
    return c[:n].reshape(p.height, p.width), a


def assert_planes(got, want, what):
    (gc, ga), (wc, wa) = got, want
    bad = gc != wc
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} counts differ, first at "
                           f"{tuple(np.argwhere(bad)[0])}: got {gc[bad][0]} want {wc[bad][0]}")
    if ga is not None:
        same = (ga.view(np.uint32) == wa.view(np.uint32)) | (np.isnan(ga) & np.isnan(wa))
        assert same.all(), f"{what}: {int((~same).sum())} ao values differ"


class Resident:
    """A context on a reference case's scene with the case's feature buffer on the device."""

    def __init__(self, case, features=None):
        self.case = case
        self.ctx = z.RenderContext(case.view, params(case.width, case.height))
        self.feat = to_dev(case.features if features is None else features)

    def ao(self, n, first=0, flags=0, trav=z.ZRT_TRAVERSAL_FAST, radius=None, **kw):
        c = self.case
        p = params(c.width, c.height, trav, c.prng, c.seed)
        a = z.ao_settings(n, float(c.radius) if radius is None else radius, first, flags)
        return run_ao(self.ctx, c.camera, p, a, self.feat, **kw)

    def close(self):
        self.ctx.close()


# ---- 1. equals the reference --------------------------------------------------------------

CASES = [(name, radius, 0) for name in ("wraps", "bubbles", "glass-inside") for radius in (math.inf, 0.75)] + \
        [("wraps", math.inf, 1), ("wraps", 0.75, 1)]


@pytest.mark.parametrize("name,radius,prng", CASES, ids=[f"{n}-{r}-prng{g}" for n, r, g in CASES])
def test_ao_equals_the_reference(scenes, name, radius, prng):
    c = ref_case(scenes, name, 24, 24, radius, prng)
    want = c.expected(0, 8)
    occ = c.occluded(0, 8)
    if name != "glass-inside" or radius != math.inf:
        assert 0.05 < occ.mean() < 0.90  # (tests/test_ao_ref.py pins the inputs)
    r = Resident(c)
    try:
        for trav in TRAVERSALS:
            assert_planes(r.ao(8, trav=trav), want, f"{name} radius {radius} prng {prng} traversal {trav}")
        got = r.ao(8, want_ao=False)  # dev_ao may be NULL
        assert np.array_equal(got[0], want[0])
    finally:
        r.close()


# ---- 2. the loaded scenes -----------------------------------------------------------------

def bunny_radius(scenes):
    """Half the extent of the hit points: at a quarter (1.71) the reference has 100 of its 2268
    rays occluded, 4.4 %; at half (3.41) 126, 5.6 % (148 at +inf)."""
    c = ref_case(scenes, 2, 32, 32)
    return float(F(0.5) * F(np.ptp(c.P, axis=0).max()))


@pytest.mark.parametrize("which,finite", [(1, False), (2, False), (2, True)],
                         ids=["scene1-list", "scene2-inf", "scene2-half-extent"])
def test_ao_on_loaded_scenes(scenes, which, finite):
    radius = bunny_radius(scenes) if finite else math.inf
    c = ref_case(scenes, which, 32, 32, radius)
    assert c.use_bvh == (which == 2)
    occ = c.occluded(0, 4)
    print(f"scene {which} radius {radius}: {occ.size} rays, {int(occ.sum())} occluded")
    assert occ.mean() >= 0.05 and (~occ).mean() >= 0.05
    want = c.expected(0, 4)
    r = Resident(c)
    try:
        for trav in TRAVERSALS if which == 2 else TRAVERSALS[:1]:
            assert_planes(r.ao(4, trav=trav), want, f"scene {which} radius {radius} traversal {trav}")
    finally:
        r.close()


# ---- 3. shape edges -----------------------------------------------------------------------

@pytest.mark.parametrize("w,h,counts", [(16, 16, (1, 3, 64, 65, 100)), (20, 20, (3, 8)), (40, 24, (3, 8))],
                         ids=["16x16", "20x20-ragged", "40x24-outside-D"])
def test_ao_shape_edges(scenes, w, h, counts):
    """Sample counts on both reductions (1, 8, 64 end in the wave; 3, 65, 100 go through the
    count plane, 65 and 100 across waves), 400 n rays (no multiple of 256, ragged tiles), and
    a frame wider than D: the columns x >= height hold 0 / 0.0."""
    c = ref_case(scenes, "wraps", w, h)
    r = Resident(c)
    try:
        for n in counts:
            want = c.expected(0, n)
            travs = TRAVERSALS if n in (3, 65) else TRAVERSALS[:1]
            for trav in travs:
                got = r.ao(n, trav=trav)
                assert_planes(got, want, f"{w}x{h} n {n} traversal {trav}")
            if w > h:
                assert (got[0][:, h:] == 0).all() and (got[1][:, h:].view(np.uint32) == 0).all()
                assert got[0][:, :h].any()
    finally:
        r.close()


# ---- 4. accumulation ----------------------------------------------------------------------

@pytest.mark.parametrize("split", [(8, 8), (3, 13)], ids=["8+8-wave", "3+13-atomic"])
def test_ao_accumulates(scenes, split):
    c = ref_case(scenes, "wraps", 24, 24)
    whole = c.expected(0, 16)
    a, b = split
    r = Resident(c)
    try:
        zero = np.zeros((24, 24), np.uint32)
        first = r.ao(a, 0, ACC, prior=zero)
        assert_planes(first, c.expected(0, a, prior=zero), f"[0, {a}) accumulated onto zeros")
        assert_planes(first, c.expected(0, a), "the first accumulated call equals a plain one")
        second = r.ao(b, a, ACC, prior=first[0])
        assert_planes(second, c.expected(a, b, prior=first[0]), f"[{a}, 16) accumulated")
        assert_planes(second, whole, "two accumulated calls equal one call of 16")
        # first_sample without the flag: that range alone
        assert_planes(r.ao(8, 8), c.expected(8, 8), "samples 8 .. 15 alone")
        assert not np.array_equal(c.expected(8, 8)[0], c.expected(0, 8)[0])
        # outside D the planes are rewritten with zeros whatever they held, flag or not
        cw = ref_case(scenes, "wraps", 40, 24)
        rw = Resident(cw)
        try:
            junk = np.full((24, 40), 9, np.uint32)
            got = rw.ao(8, 0, ACC, prior=junk)
            assert_planes(got, cw.expected(0, 8, prior=junk), "40x24 accumulated onto nines")
            assert (got[0][:, 24:] == 0).all()
        finally:
            rw.close()
    finally:
        r.close()


# ---- 5. consistency with zrt_ctx_occluded -------------------------------------------------

def test_ao_equals_occluded_on_the_gpus_own_features(scenes):
    """Scene 2, 64 x 64, n = 16: the rays are rebuilt in numpy from the GPU's own feature
    buffer and sent through zrt_ctx_occluded; their per-pixel sums are dev_clear."""
    import torch
    s = scenes(2)
    w = h = 64
    n = 16
    p = params(w, h)
    ctx = z.RenderContext(s, p)
    try:
        feat = torch.zeros(w * h * 8, dtype=torch.float32, device="cuda")
        ctx.features(s.camera, p, feat.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        f = feat.cpu().numpy().reshape(h, w, 8)
        c = AO.AoCase(O, s.view, s.camera, w, h, features=f)
        assert 1000 < len(c.ys) < w * h
        o, d = c.rays(0, n)
        rays = to_dev(np.concatenate([o, d], 1).astype(F))
        out = torch.zeros(len(o), dtype=torch.uint8, device="cuda")
        ctx.occluded(p, rays.data_ptr(), 0, len(o), out.data_ptr())
        ctx.sync()
        torch.cuda.synchronize()
        occ = out.cpu().numpy().reshape(-1, n) != 0
        assert 0.05 < occ.mean() < 0.95
        want = np.zeros((h, w), np.uint32)
        want[c.miss] = n
        want[c.ys, c.xs] = (~occ).sum(1)
        got, ao = run_ao(ctx, s.camera, p, z.ao_settings(n), feat)
        assert np.array_equal(got, want)
        assert np.array_equal(ao.view(np.uint32), (want.astype(F) / F(n)).view(np.uint32))
        assert ctx.ao_ms() > 0.0 and ctx.ao_ms() == ctx.query_ms()
    finally:
        ctx.close()


# ---- 6. synthetic features ----------------------------------------------------------------

@pytest.mark.parametrize("n", [8, 3], ids=["wave", "atomic"])
def test_ao_poisoned_pixels_and_garbage_misses(scenes, n):
    base = ref_case(scenes, "wraps", 24, 24)
    f = base.features.copy()
    hits = list(zip(base.ys, base.xs))
    (y0, x0), (y1, x1), (y2, x2), (y3, x3) = hits[0], hits[len(hits) // 3], hits[len(hits) // 2], hits[-1]
    f[y0, x0, 1] = np.nan          # a lane of N
    f[y1, x1, 3] = np.nan          # t
    f[y2, x2, 0:4] = np.nan        # the whole record, as a device error leaves it ...
    f[y2, x2, 4:8] = np.nan        # ... id included (NaN bits are not 0: no miss)
    f[y3, x3, 0:4] = (1e30, np.nan, -5.0, -np.inf)  # garbage N and t ...
    f[y3, x3, 7] = 0.0                               # ... on a miss
    c = AO.AoCase(O, base.view, base.camera, 24, 24, features=f)
    assert c.poison.sum() == 3 and c.miss[y3, x3]
    r = Resident(c)
    try:
        want = c.expected(0, n)
        got = r.ao(n)
        assert_planes(got, want, "poisoned features")
        for y, x in ((y0, x0), (y1, x1), (y2, x2)):
            assert got[0][y, x] == AO.POISON and np.isnan(got[1][y, x])
        assert got[0][y3, x3] == n and got[1][y3, x3] == 1.0
        assert int((got[0] == AO.POISON).sum()) == 3 and int(np.isnan(got[1]).sum()) == 3
        # under accumulation a poisoned count stays poisoned, also once the pixel's features are clean
        again = r.ao(n, n, ACC, prior=got[0])
        assert_planes(again, c.expected(n, n, prior=got[0]), "accumulated onto poisoned counts")
        clean = Resident(base)
        try:
            healed = clean.ao(n, n, ACC, prior=got[0])
            assert_planes(healed, base.expected(n, n, prior=got[0]), "clean features, poisoned plane")
            assert healed[0][y0, x0] == AO.POISON and np.isnan(healed[1][y0, x0])
        finally:
            clean.close()
    finally:
        r.close()


# ---- 7. refusals --------------------------------------------------------------------------

def test_ao_refusals(scenes):
    import torch
    s = scenes(2)
    p = params(16, 16)
    ctx = z.RenderContext(s, p)
    feat = torch.zeros(16 * 16 * 8 + 8, dtype=torch.float32, device="cuda")
    clear = torch.zeros(16 * 16 + 8, dtype=torch.int32, device="cuda")
    fp, cp = feat.data_ptr(), clear.data_ptr()
    ok = z.ao_settings(4)
    try:
        ctx.ao(s.camera, p, ok, fp, cp, cp)
        ctx.sync()
        for call in (lambda: ctx.ao(s.camera, p, z.ao_settings(0), fp, cp),
                     lambda: ctx.ao(s.camera, p, z.ao_settings(1025), fp, cp),
                     lambda: ctx.ao(s.camera, p, z.ao_settings(8, first_sample=65536 - 7), fp, cp),
                     lambda: ctx.ao(s.camera, p, z.ao_settings(4, math.nan), fp, cp),
                     lambda: ctx.ao(s.camera, p, z.ao_settings(4, 0.001), fp, cp),
                     lambda: ctx.ao(s.camera, p, z.ao_settings(4, -1.0), fp, cp),
                     lambda: ctx.ao(s.camera, p, z.ao_settings(4, flags=2), fp, cp),
                     lambda: ctx.ao(s.camera, p, ok, 0, cp),
                     lambda: ctx.ao(s.camera, p, ok, fp, 0),
                     lambda: ctx.ao(s.camera, p, ok, fp + 4, cp),     # features: 16 bytes
                     lambda: ctx.ao(s.camera, p, ok, fp, cp + 2),
                     lambda: ctx.ao(s.camera, p, ok, fp, cp, cp + 1),
                     lambda: ctx.ao(s.camera, params(16, 24), ok, fp, cp),   # height > width
                     lambda: ctx.ao(s.camera, params(16, 16, trav=3), ok, fp, cp),
                     lambda: ctx.ao(s.camera, params(16, 16, prng=2), ok, fp, cp),
                     lambda: ctx.ao(s.camera, params(16, 16, bounded_volume_hierarchy=False), ok, fp, cp),
                     lambda: ctx.ao(s.camera, params(16, 16, device=1), ok, fp, cp)):
            with pytest.raises(z.ZrtError) as e:
                call()
            assert e.value.code == _ffi.ZRT_E_INVALID
        ctx.sync()  # nothing was enqueued, nothing is pending
    finally:
        ctx.close()


# ---- 8. the device error convention -------------------------------------------------------

@pytest.mark.parametrize("n", [4, 3], ids=["wave", "atomic"])
def test_ao_stack_overflow_is_reported(scenes, n, monkeypatch):
    """A stack too small for the tree (ZRT_DEBUG_STACK_CAP, as test_query_stack_overflow_is_reported
    uses it): 0xFFFFFFFF / NaN in D, 0 / 0.0 outside, ZRT_E_UNSUPPORTED once, then a correct answer."""
    # scene 2 in a 40 x 32 frame: the 32 x 32 frame's first hits (any finite record serves: AO is
    # a function of the buffer), columns 32 .. 39 outside D
    if "overflow" not in _KEEP:
        c = ref_case(scenes, 2, 32, 32)
        wide = np.zeros((32, 40, 8), F)
        wide[:, :32] = c.features
        _KEEP["overflow"] = AO.AoCase(O, c.view, c.camera, 40, 32, features=wide)
    cw = _KEEP["overflow"]
    want = cw.expected(0, n)
    assert (want[0][:, 32:] == 0).all() and len(np.unique(want[0][:, :32])) >= 3
    r = Resident(cw)
    try:
        monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
        got = r.ao(n, sync=False)
        with pytest.raises(z.ZrtError) as e:
            r.ctx.sync()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and "overflow" in str(e.value)
        assert (got[0][:, :32] == AO.POISON).all() and np.isnan(got[1][:, :32]).all()
        assert (got[0][:, 32:] == 0).all() and (got[1][:, 32:] == 0).all()
        r.ctx.sync()  # reported once
        monkeypatch.delenv("ZRT_DEBUG_STACK_CAP")
        after = r.ao(n)
        assert_planes(after, want, "after the error")
    finally:
        r.close()


# ---- 9. no interference -------------------------------------------------------------------

def test_ao_leaves_runs_renders_and_streams_alone(scenes):
    import torch
    s = scenes(2)
    c = ref_case(scenes, 2, 32, 32)
    want = c.expected(0, 4)
    feat = to_dev(c.features)
    p = z.RenderParams(32, 32, 8, 6, sample_chunk=2)
    pa = params(32, 32)

    def run(with_ao):
        ctx = z.RenderContext(s, p)
        try:
            tiles = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
            frame = torch.zeros(32 * 32 * 3, dtype=torch.float32, device="cuda")
            ctx.accum_begin(s.camera, p)
            ctx.accum_pass(4, tiles.data_ptr())
            if with_ao:
                assert_planes(run_ao(ctx, s.camera, pa, z.ao_settings(4), feat), want, "between two passes")
            ctx.accum_pass(4, tiles.data_ptr())
            ctx.assemble(p, tiles.data_ptr(), frame.data_ptr())
            ctx.sync()
            torch.cuda.synchronize()
            img, st = frame.cpu().numpy().reshape(32, 32, 3).copy(), ctx.stats()
            if with_ao:
                # on a torch stream, then a plain render that must be the oracle's
                stream = torch.cuda.Stream()
                assert_planes(run_ao(ctx, s.camera, pa, z.ao_settings(4), feat, stream=stream.cuda_stream), want,
                              "on a torch stream")
                rp = z.RenderParams(16, 16, 2, 8)
                t2 = torch.zeros(ctx.tile_count(rp) * 64 * 3, dtype=torch.float32, device="cuda")
                f2 = torch.zeros(16 * 16 * 3, dtype=torch.float32, device="cuda")
                ctx.render_tiles(s.camera, rp, t2.data_ptr())
                ctx.assemble(rp, t2.data_ptr(), f2.data_ptr())
                ctx.sync()
                torch.cuda.synchronize()
                ref, rst = O.render(s.view, s.camera, rp)
                assert np.array_equal(f2.cpu().numpy().reshape(16, 16, 3).view(np.uint32), ref.view(np.uint32))
                assert ctx.stats()["rays_processed"] == rst["rays_processed"]
                assert_planes(run_ao(ctx, s.camera, pa, z.ao_settings(4), feat), want, "after a render")
            return img, st
        finally:
            ctx.close()

    plain, st0 = run(False)
    mixed, st1 = run(True)
    assert np.array_equal(plain.view(np.uint32), mixed.view(np.uint32))
    assert st0["rays_processed"] == st1["rays_processed"]
    ref, _ = O.render(s.view, s.camera, p)
    assert np.array_equal(plain.view(np.uint32), ref.view(np.uint32))


# ---- 10. the one-shot call and the CLI ----------------------------------------------------

def test_render_ao_equals_the_context_path(scenes):
    s = scenes(2)
    c = ref_case(scenes, 2, 32, 32)
    for trav in TRAVERSALS:
        ao, clear, feat = z.render_ao(s, s.camera, params(32, 32, trav), 4)
        assert np.array_equal(feat.view(np.uint32), c.features.view(np.uint32))
        assert_planes((clear, ao), c.expected(0, 4), f"one-shot, traversal {trav}")
    radius = bunny_radius(scenes)
    ao, clear, _ = z.render_ao(s, s.camera, params(32, 32), 4, radius=radius)
    assert_planes((clear, ao), ref_case(scenes, 2, 32, 32, radius).expected(0, 4), "one-shot, finite radius")
    ao, clear, _ = z.render_ao(s, s.camera, params(32, 32), 4, first_sample=4)
    assert_planes((clear, ao), c.expected(4, 4), "one-shot, first_sample 4")
    s1 = scenes(1)
    ao, clear, _ = z.render_ao(s1, s1.camera, params(32, 32), 4)
    assert_planes((clear, ao), ref_case(scenes, 1, 32, 32).expected(0, 4), "one-shot, surface list")
    with pytest.raises(z.ZrtError) as e:
        z.render_ao(s, s.camera, params(32, 32), 0)
    assert e.value.code == _ffi.ZRT_E_INVALID


def test_cli_ao(scenes, tmp_path):
    """zrt-raytrace 32 32 2 5 2 out.png with ZRT_AO_SAMPLES / ZRT_AO_OUT: the AO plane as a grey
    PNG beside the frame, which is the one written without them."""
    s = scenes(2)
    c = ref_case(scenes, 2, 32, 32)
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    drop = ("ZRT_PASS_SAMPLES", "ZRT_DEVICES", "ZRT_ADAPTIVE_TOL", "ZRT_DENOISE", "ZRT_TEMPORAL_FRAMES",
            "ZRT_AO_SAMPLES", "ZRT_AO_RADIUS", "ZRT_AO_OUT")
    env = {k: v for k, v in os.environ.items() if k not in drop}
    r = subprocess.run([exe, "32", "32", "2", "5", "2", str(tmp_path / "plain.png")], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "Ambient occlusion" not in r.stderr
    for radius in (None, bunny_radius(scenes)):
        e2 = {**env, "ZRT_AO_SAMPLES": "4", "ZRT_AO_OUT": str(tmp_path / "ao.png")}
        if radius is not None:
            e2["ZRT_AO_RADIUS"] = repr(radius)
        r = subprocess.run([exe, "32", "32", "2", "5", "2", str(tmp_path / "out.png")], env=e2, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "  Ambient occlusion:     4 rays per pixel" in r.stderr
        assert (tmp_path / "out.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
        want = ref_case(scenes, 2, 32, 32, math.inf if radius is None else radius).expected(0, 4)[1]
        z.write_png(str(tmp_path / "want.png"), np.repeat(want[..., None], 3, 2))
        assert (tmp_path / "ao.png").read_bytes() == (tmp_path / "want.png").read_bytes()
    assert len(set(np.unique(c.expected(0, 4)[1]))) >= 4  # (a plane with grey levels, not a flat one)

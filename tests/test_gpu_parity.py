"""GPU parity: the HIP path (through the C ABI) against the oracle.

Bar: bit-exact.  In counter-RNG mode the kernel and the oracle draw the same
random numbers and execute the same f32 operations (both -ffp-contract=off,
both with correctly rounded div/sqrt and the same restated transcendentals),
so images and progress counters must be identical — NaN compares equal to NaN.

Run on an MI355X: ``pytest -m gpu``.
"""
import json
import os

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

COUNTERS = ("recursion_depth_hits", "reflections", "background_hits", "rays_processed",
            "pixels_processed", "samples_processed")


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a) & np.isnan(b)
    eq = (a.view(np.uint32) == b.view(np.uint32)) | nan
    return eq


def assert_bit_exact(gpu, ref):
    eq = same_bits(gpu, ref)
    if not eq.all():
        bad = np.argwhere(~eq.reshape(gpu.shape[0], gpu.shape[1], 3).all(axis=2))
        y, x = bad[0]
        raise AssertionError(f"{len(bad)} pixels differ; first at (x={x}, y={y}): "
                             f"gpu={gpu[y, x]} oracle={ref[y, x]}; max|d|="
                             f"{np.nanmax(np.abs(gpu - ref))}")


# ---- device building blocks ---------------------------------------------------

@pytest.mark.parametrize("prng", [z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256])
def test_device_rng_matches_oracle(golden, prng):
    for key in (0, 42, 0x123456789ABCDEF, int(golden["streams"]["counter_keys_seed42"][3]["key"])):
        np.testing.assert_array_equal(z.debug_rng(prng, key, 64), O.prng_u64(prng, key, 64))


def test_device_math_bit_exact():
    rng = np.random.default_rng(7)
    n = 4096
    phi = (np.float32(6.2831855) * rng.random(n, dtype=np.float32)).astype(np.float32)
    for fn, name in ((0, "sin"), (1, "cos")):
        assert same_bits(z.debug_math(fn, phi), O.math1(name, phi)).all(), name
    c = np.concatenate([rng.uniform(-1, 1, n).astype(np.float32),
                        np.array([-1, 1, 0, -0.0, 0.5, -0.5, 1e-9, 1.0000001, np.nan], np.float32)])
    assert same_bits(z.debug_math(2, c), O.math1("acos", c)).all(), "acos"
    a = np.concatenate([rng.normal(0, 5, n).astype(np.float32), np.array([0, 1e30, -1e-30], np.float32)])
    assert same_bits(z.debug_math(3, a), O.math1("atan", a)).all(), "atan"
    ys, xs = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    ys[:4] = [0, -0.0, 1, 0]
    xs[:4] = [-1, -1, 0, 1]
    assert same_bits(z.debug_math(5, ys, xs), O.math2("atan2", ys, xs)).all(), "atan2"
    # magnitudes over the whole exponent range: the short divisions inside atan / atan2
    # (dev::div_rn) fall back to IEEE `/` where an operand or quotient leaves [2^-50, 2^50]
    mag = lambda k: (rng.choice([-1, 1], k) * 10.0 ** rng.uniform(-40, 38, k)).astype(np.float32)
    ys, xs = mag(n), mag(n)
    assert same_bits(z.debug_math(5, ys, xs), O.math2("atan2", ys, xs)).all(), "atan2 wide"
    aw = mag(n)
    assert same_bits(z.debug_math(3, aw), O.math1("atan", aw)).all(), "atan wide"
    cw = np.concatenate([(rng.choice([-1, 1], n) * 10.0 ** rng.uniform(-45, 0, n)).astype(np.float32),
                         np.nextafter(np.float32([1, -1]), np.float32(0))])
    assert same_bits(z.debug_math(2, cw), O.math1("acos", cw)).all(), "acos wide"
    p = np.concatenate([rng.random(n, dtype=np.float32), np.array([0, 1, 2, 1e-7, 2 ** -24], np.float32)])
    assert same_bits(z.debug_math(6, p), O.math2("pow", p, np.full_like(p, 5.0))).all(), "pow5"
    # IEEE correctly rounded sqrt and division (HIP's default for f32)
    s = np.abs(rng.normal(0, 100, n)).astype(np.float32)
    assert same_bits(z.debug_math(4, s), np.sqrt(s)).all(), "sqrt"
    den = rng.normal(0, 3, n).astype(np.float32)
    assert same_bits(z.debug_math(7, a[:n], den), (a[:n] / den).astype(np.float32)).all(), "div"


def _edge_floats():
    f = np.float32
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2 ** -126, -(2 ** -126), 2 ** -149,
                         np.finfo(f).max, -np.finfo(f).max, 2.0 ** 126, 2.0 ** 125 * 1.9999999, 2 ** -50,
                         2 ** 50, 2 ** -51, 2 ** 51, 1e-6, 1.52], f)
    bits = np.random.default_rng(11).integers(0, 2 ** 32, 1 << 16, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([specials, bits.view(f)])


def test_short_divisions_equal_ieee_on_edges():
    """The kernel's short reciprocal / division / sqrt sequences (device_math.hpp
    rcp_rn, div_rn, sqrt_rn: v_rcp + Newton step, Markstein's correction, v_sqrt + FMA
    fix-up, range-guarded) give IEEE results bit for bit, on special values and
    random bit patterns."""
    x = _edge_floats()
    with np.errstate(all="ignore"):
        assert same_bits(z.debug_math(8, x), (np.float32(1) / x).astype(np.float32)).all(), "rcp_rn"
        y = np.roll(x, 7)
        assert same_bits(z.debug_math(9, x, y), (x / y).astype(np.float32)).all(), "div_rn"
        assert same_bits(z.debug_math(9, x, y), z.debug_math(7, x, y)).all(), "div_rn vs device IEEE"
        assert same_bits(z.debug_math(4, x), np.sqrt(x)).all(), "sqrt_rn"


def test_short_divisions_device_self_check():
    """zrt_debug_division: the reciprocal and sqrt over all 2^32 inputs, and division, unit(),
    1/d and the jitter quotient over 2^28 hashed inputs each (signed zeros,
    subnormals, inf, NaN, every exponent, near-midpoint quotients), against the
    device's own IEEE `/`: no mismatch."""
    counts = z.debug_division(1 << 28)
    assert counts == {"rcp_sqrt_all_2p32": 0, "div": 0, "unit": 0, "inv_dir": 0, "jitter": 0}, counts


# ---- whole-frame parity ---------------------------------------------------------

CASES = [
    # (scene, width, height, spp, depth)
    (1, 48, 48, 8, 30),    # seven spheres, list mode (C1/C2 scene)
    (2, 32, 32, 4, 20),    # bunny + ball, BVH (C4 scene)
    (3, 32, 32, 4, 20),    # teapot + ball (C3 scene)
    (4, 24, 24, 4, 20),    # teapot + ball circle: image-textured lambertian, hollow metal sphere
    (0, 24, 24, 4, 20),    # man + ball
]


@pytest.mark.parametrize("traversal", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE, z.ZRT_TRAVERSAL_BINARY],
                         ids=["fast", "reference", "binary"])
@pytest.mark.parametrize("case", CASES, ids=[f"scene{c[0]}" for c in CASES])
def test_render_bit_exact_vs_oracle(scenes, case, traversal):
    idx, w, h, spp, depth = case
    s = scenes(idx)
    p = z.RenderParams(w, h, spp, depth, traversal=traversal)
    gpu, gs = z.render(s, s.camera, p)
    ref, rs = O.render(s.view, s.camera, p)
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k
    # the diagnostic flavour renders the same image and counts rays directly
    p.flags = z.ZRT_FLAG_STATS
    gpu2, gs = z.render(s, s.camera, p)
    assert same_bits(gpu, gpu2).all()
    for k in COUNTERS:
        assert gs[k] == rs[k], k
    if traversal == z.ZRT_TRAVERSAL_REFERENCE and rs["used_bvh"]:
        # the same DFS with the same slab tests visits the same nodes
        assert gs["node_visits"] == rs["node_visits"]


def set_loop(monkeypatch, loop):
    """Force one FAST sampling loop: lockstep (render_loop), wavefront
    (render_loop_wf) or path pool (render_loop_pool)."""
    monkeypatch.setenv("ZRT_WF", "1" if loop == "wavefront" else "0")
    monkeypatch.setenv("ZRT_POOL", "1" if loop == "pool" else "0")


@pytest.mark.parametrize("loop", ["lockstep", "wavefront", "pool"])
@pytest.mark.parametrize("case", [c for c in CASES if c[0] != 1], ids=[f"scene{c[0]}" for c in CASES if c[0] != 1])
def test_render_loops_bit_exact(scenes, case, loop, monkeypatch):
    """The three FAST sampling loops (render_loop, the wavefront render_loop_wf and
    the path-pool render_loop_pool) on every BVH scene, with more
    samples per pixel and a chunk that splits them: images, counters and
    per-scanline counters equal the oracle's."""
    set_loop(monkeypatch, loop)
    idx, w, h, _, depth = case
    s = scenes(idx)
    p = z.RenderParams(w, h, 24, depth, sample_chunk=7)
    gpu, gs, rows = z.render_progress(s, s.camera, p)
    ref, rs, rrows = O.render_scanlines(s.view, s.camera, p)
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k
    np.testing.assert_array_equal(rows, rrows)


@pytest.mark.parametrize("lanes", ["items", "wave"])
@pytest.mark.parametrize("w,h,spp,chunk", [(40, 40, 24, 7), (45, 30, 9, 4)])
def test_list_loops_bit_exact(scenes, lanes, w, h, spp, chunk, monkeypatch):
    """The surface-list loops on scene 1 (seven spheres, glass and metal, depth 30:
    config C2's scene): per-lane work items (render_loop_list, the default) and
    the wave-unit loop (render_loop MODE 0, ZRT_LIST_LANES=0), with chunks that
    split the samples and a ragged frame: images, counters and per-scanline
    counters equal the oracle's."""
    monkeypatch.setenv("ZRT_LIST_LANES", "1" if lanes == "items" else "0")
    s = scenes(1)
    p = z.RenderParams(w, h, spp, 30, sample_chunk=chunk)
    gpu, gs, rows = z.render_progress(s, s.camera, p)
    ref, rs, rrows = O.render_scanlines(s.view, s.camera, p)
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k
    np.testing.assert_array_equal(rows, rrows)
    assert gs["sampling_loop"] == (6 if lanes == "items" else 0)
    img2, gs2 = z.render(s, s.camera, p)  # without the scanline flag: counters from the wave sums
    assert_bit_exact(img2, ref)
    for k in COUNTERS:
        assert gs2[k] == rs[k], k


def test_c5_substitute_bit_exact(scenes):
    """Scene 6, the stated C5 substitute: 1.6 M subdivided teapot triangles
    (reference BVH 1 894 803 nodes, depth 39) with image-textured lambertians on both surfaces, so the
    scene and textures exceed L2.  FAST and REFERENCE traversal against the
    oracle (whose reference-order traversal of this tree bounds the size)."""
    s = scenes(6)
    p = z.RenderParams(16, 16, 1, 4)
    ref, rs = O.render(s.view, s.camera, p)
    assert rs["used_bvh"] and rs["bvh_nodes"] == 1_894_803
    for trav in (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE):
        p.traversal = trav
        gpu, gs = z.render(s, s.camera, p)
        assert_bit_exact(gpu, ref)
        for k in COUNTERS:
            assert gs[k] == rs[k], k


@pytest.mark.parametrize("loop,rows", [("wavefront", None), ("wavefront", "2"), ("lockstep", "2"), ("pool", None),
                                       ("pool", "2")])
def test_c5_substitute_depth20_vs_golden(scenes, loop, rows, monkeypatch):
    """the C5 path at its real depth.  Scene 6 at 32x32 x 2 spp,
    max depth 20, 1-sample chunks, against the oracle's frame, progress counters
    and per-scanline counters (tests/golden/c5_depth20.npz, made by
    tests/golden/make_c5_golden.py: the oracle needs ~160 s for it).  The
    path-pool loop (the C5 default), the wavefront loop and the lockstep loop;
    rows="2" forces the
    FAST stack onto its global rows past 2 LDS rows, and every run keeps no
    attenuation row in LDS (ZRT_ATT_LDS_ROWS=0), so both deep-tree paths to
    global memory are taken - checked with the STATS counters kAttWrites and
    kStackOvfWrites."""
    import os
    import torch
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c5_depth20.npz"))
    w, h, spp, depth, chunk = (int(x) for x in g["params"])
    set_loop(monkeypatch, loop)
    monkeypatch.setenv("ZRT_ATT_LDS_ROWS", "0")
    if rows:
        monkeypatch.setenv("ZRT_STACK_LDS_ROWS", rows)
    s = scenes(6)
    p = z.RenderParams(w, h, spp, depth, sample_chunk=chunk)
    gpu, gs, grows = z.render_progress(s, s.camera, p)
    assert_bit_exact(gpu, g["image"])
    for name, v in zip(g["counter_names"], g["counters"]):
        assert gs[str(name)] == int(v), name
    np.testing.assert_array_equal(grows, g["rows"])
    assert gs["reflections"] > 0 and gs["recursion_depth_hits"] >= 0
    # the same frame from a context, diagnostic flavour: rows past LDS were used
    ctx = z.RenderContext(s, p)
    buf = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
    ps = z.RenderParams(**{**p.__dict__, "flags": z.ZRT_FLAG_STATS})
    ctx.render_tiles(s.camera, ps, buf.data_ptr())
    ctx.sync()
    dc = ctx.debug_counters(32)
    assert dc[28] > 0, "no attenuation row reached global memory"  # kAttWrites
    if rows:
        assert dc[30] > 0, "no stack entry reached the global rows"  # kStackOvfWrites
    ctx.close()


def test_nonsquare_and_ragged_tiles(scenes):
    """height < width: raytrace.zig:168 leaves columns x >= height black; 8x8
    tiles overhang both edges (37 x 21)."""
    s = scenes(1)
    p = z.RenderParams(37, 21, 3, 12)
    gpu, gs = z.render(s, s.camera, p)
    ref, rs = O.render(s.view, s.camera, p)
    assert_bit_exact(gpu, ref)
    assert np.all(gpu[:, 21:] == 0)
    assert gs["pixels_processed"] == 21 * 21 == rs["pixels_processed"]


@pytest.mark.parametrize("max_depth", [0, 1, 2])
def test_shallow_depths(scenes, max_depth):
    """depth <= 0 returns black and counts a recursion-limit hit (raytrace.zig:64-68)."""
    s = scenes(2)
    p = z.RenderParams(16, 16, 2, max_depth)
    gpu, gs = z.render(s, s.camera, p)
    ref, rs = O.render(s.view, s.camera, p)
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k


def test_xoshiro_and_seed(scenes):
    s = scenes(1)
    for prng, seed in ((z.ZRT_PRNG_XOSHIRO256, 42), (z.ZRT_PRNG_XOROSHIRO128, 7)):
        p = z.RenderParams(24, 24, 4, 30, prng=prng, seed=seed)
        assert_bit_exact(z.render(s, s.camera, p)[0], O.render(s.view, s.camera, p)[0])


def test_no_bvh_flag_uses_list(scenes):
    """bounded_volume_hierarchy = false: the surface list path on a mesh scene."""
    s = scenes(4)
    p = z.RenderParams(8, 8, 2, 6, bounded_volume_hierarchy=False)
    gpu, gs = z.render(s, s.camera, p)
    ref, rs = O.render(s.view, s.camera, p)
    assert gs["used_bvh"] == 0
    assert_bit_exact(gpu, ref)


def test_deterministic(scenes):
    s = scenes(2)
    p = z.RenderParams(64, 64, 8, 20)
    a, _ = z.render(s, s.camera, p)
    b, _ = z.render(s, s.camera, p)
    assert same_bits(a, b).all()


# ---- tile partition (multi-GPU path on one device) ----------------------------------

def render_partitioned(scene, p_base, world):
    import torch
    ctx = z.RenderContext(scene, p_base)
    parts = []
    for rank in range(world):
        p = z.RenderParams(**{**p_base.__dict__, "rank": rank, "world_size": world})
        n = ctx.tile_count(p)
        buf = torch.empty(n * 64 * 3, dtype=torch.float32, device="cuda")
        ctx.render_tiles(scene.camera, p, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        parts.append(buf)
    gathered = torch.cat(parts)
    pw = z.RenderParams(**{**p_base.__dict__, "rank": 0, "world_size": world})
    frame = torch.empty(p_base.height * p_base.width * 3, dtype=torch.float32, device="cuda")
    ctx.assemble(pw, gathered.data_ptr(), frame.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = frame.cpu().numpy().reshape(p_base.height, p_base.width, 3)
    ctx.close()
    return out


@pytest.mark.parametrize("world", [2, 3, 8])
def test_tile_partition_invariance(scenes, world):
    """1 vs N ranks: bitwise-identical frames (SURVEY §8c protocol 2)."""
    s = scenes(2)
    p = z.RenderParams(40, 40, 4, 20)
    one = render_partitioned(s, p, 1)
    many = render_partitioned(s, p, world)
    assert same_bits(one, many).all()
    assert_bit_exact(one, O.render(s.view, s.camera, p)[0])


@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0, 0, 0, 0, 0, 0]])
@pytest.mark.parametrize("scene_index", [1, 2])
def test_render_multi_bit_exact(scenes, scene_index, devices):
    """zrt_render_multi (one process, several GPUs): [0] runs the RCCL gather
    (ncclCommInitAll + ncclGather with one rank); a repeated device runs that
    many ranks on one GPU (device-copy gather).  Same image and counters as
    zrt_render, and as the oracle."""
    s = scenes(scene_index)
    p = z.RenderParams(40, 40, 4, 30 if scene_index == 1 else 20)
    one, st1 = z.render(s, s.camera, p)
    multi, stm = z.render_multi(s, s.camera, p, devices)
    assert same_bits(one, multi).all()
    for k in COUNTERS:
        assert st1[k] == stm[k], k
    assert stm["n_gpus"] == 1
    assert_bit_exact(multi, O.render(s.view, s.camera, p)[0])


def test_render_multi_errors(scenes):
    s = scenes(2)
    p = z.RenderParams(16, 16, 1, 20)
    with pytest.raises(z.ZrtError) as e:
        z.render_multi(s, s.camera, p, [])
    assert e.value.code == z._ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:
        z.render_multi(s, s.camera, p, [0, 4096])
    assert e.value.code == z._ffi.ZRT_E_NODEVICE


# ---- the bench configuration, checked through size-independent properties ----------

def test_bench_config_properties(scenes):
    """Bunny at the bench's 2048^2 resolution (16 spp here): counter identities,
    value range, and bit-exact rows against the oracle."""
    s = scenes(2)
    p = z.RenderParams(2048, 2048, 16, 20)
    img, st = z.render(s, s.camera, p)
    assert st["pixels_processed"] == 2048 * 2048
    assert st["samples_processed"] == 2048 * 2048 * 16
    assert st["samples_processed"] + st["reflections"] == st["rays_processed"] + st["recursion_depth_hits"]
    assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
    for y in (0, 1024, 2047):  # one full row each, 2048 x 16 samples
        ref, _ = O.render(s.view, s.camera, p, rows=(y, y + 1))
        assert_bit_exact(img[y:y + 1], ref[y:y + 1])


@pytest.mark.parametrize("chunk", [1, 7, 64, 100])
def test_sample_chunks(scenes, chunk):
    """zrt.h sample_chunk: chunk sums in chunk order; chunk >= spp is the
    reference's single sequential sum (raytrace.zig:177)."""
    s = scenes(1)
    p = z.RenderParams(16, 16, 100, 30, sample_chunk=chunk)
    gpu, gs = z.render(s, s.camera, p)
    ref, rs = O.render(s.view, s.camera, p)
    assert_bit_exact(gpu, ref)
    assert gs["samples_processed"] == rs["samples_processed"] == 16 * 16 * 100


def _texture_scene(rng):
    """Two image-textured spheres over a ground sphere: one image exact 8-bit
    (stored as RGBX8 on the device), one with arbitrary f32 values (kept f32)."""
    from zraytrace_amd import _ffi
    import ctypes as C
    img8 = (rng.integers(0, 256, (37, 53, 3)).astype(np.float32) / np.float32(255.0)).astype(np.float32)
    imgf = rng.random((29, 41, 3), dtype=np.float32)
    imgs = (_ffi.Image * 2)(_ffi.Image(53, 37, img8.ctypes.data_as(C.POINTER(C.c_float))),
                            _ffi.Image(41, 29, imgf.ctypes.data_as(C.POINTER(C.c_float))))
    texs = (_ffi.Texture * 3)(_ffi.Texture(_ffi.ZRT_TEX_IMAGE, 0, _ffi.Vec3(0, 0, 0), 0.25, 0.1),
                              _ffi.Texture(_ffi.ZRT_TEX_IMAGE, 1, _ffi.Vec3(0, 0, 0), 0.0, 0.0),
                              _ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0.4, 0.7, 0.3), 0.0, 0.0))
    mats = (_ffi.Material * 3)(_ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 0, 0.0),
                               _ffi.Material(_ffi.ZRT_MAT_METAL, 1, 0.0),
                               _ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 2, 0.0))
    prims = (_ffi.Prim * 3)()
    for i, (c, r, m) in enumerate((((1.0, -101.5, 4.0), 100.0, 2), ((-1.2, 0.0, 4.0), 1.0, 0),
                                   ((1.3, 0.0, 4.5), 1.1, 1))):
        prims[i].kind = _ffi.ZRT_PRIM_SPHERE
        prims[i].material = m
        prims[i].center = _ffi.Vec3(*c)
        prims[i].radius = r
    scene = _ffi.Scene(prims, 3, 3, mats, texs, 3, 2, imgs)
    scene._keep = (prims, mats, texs, imgs, img8, imgf)
    return scene


def test_texel_stores_bit_exact():
    """8-bit-exact images take the RGBX8 + table path, others stay f32; both
    must give the oracle's image (texture.zig:20-74 on f32 values)."""
    import ctypes as C
    s = _texture_scene(np.random.default_rng(11))
    cam = z.camera_init((0, 0, -3), (0, 0, 4), (0, 1, 0), 45.0, 1.0)
    p = z.RenderParams(32, 32, 4, 8)
    gpu, gs = z.render(C.pointer(s), cam, p)
    ref, rs = O.render(C.pointer(s), cam, p)
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k
    assert gs["texel_bytes"] == 12  # one f32 image in the scene


_MM_ORACLE = {}  # (bvh, max_depth, prng) -> the oracle's frame of the many-materials scene


def _mm_cases():
    """(bvh, max_depth, pool, prng); the two cases this test had before it covered the
    shallow depths (depth 6, default PRNG, no ZRT_POOL) keep their ids, "True" and "False"."""
    combos = [(b, d, False) for b in (True, False) for d in (0, 1, 2, 6)] + [(True, 1, True), (True, 6, True)]
    out = []
    for bvh, depth, pool in combos:
        for name, prng in (("xoroshiro", z.ZRT_PRNG_XOROSHIRO128), ("xoshiro", z.ZRT_PRNG_XOSHIRO256)):
            first = depth == 6 and not pool and name == "xoroshiro"
            out.append(pytest.param(bvh, depth, pool, prng,
                                    id=str(bvh) if first else f"{bvh}-{depth}-{'pool-' if pool else ''}{name}"))
    return out


@pytest.mark.parametrize("bvh,max_depth,pool,prng", _mm_cases())
def test_material_table_past_lds_share(bvh, max_depth, pool, prng, monkeypatch):
    """The lockstep and list-lane loops read the material table from LDS only
    (through LDS-typed pointers); a table past their LDS share renders on the loop that reads
    it from global memory (FAST: the wavefront loop; list: the wave-unit loop), with
    no tile schedule (its probe is the lockstep loop) - the oracle's frame either way.
    At max_depth 0 no loop shades and the wavefront loop (written for max_depth >= 1:
    it would trace, and its first scatter would write attenuation row 1 of a one-row
    buffer) must not be chosen: the lockstep loop renders the black frame.  With
    ZRT_POOL=1 the path pool, which reads the table from global memory too, renders it."""
    import ctypes as C
    import many_materials as M
    if pool:
        monkeypatch.setenv("ZRT_POOL", "1")
    s = M.many_materials_scene()
    cam = M.camera()
    p = z.RenderParams(16, 16, 128 if bvh else 4, max_depth, bounded_volume_hierarchy=bvh, prng=prng)
    if (bvh, max_depth, prng) not in _MM_ORACLE:
        _MM_ORACLE[bvh, max_depth, prng] = O.render(C.pointer(s), cam, p)
    ref, rs = _MM_ORACLE[bvh, max_depth, prng]
    # (the shallow cases are not vacuous: paths reach the depth limit at every depth rendered)
    assert rs["recursion_depth_hits"] > 0
    if max_depth == 0:
        assert rs["recursion_depth_hits"] == rs["samples_processed"] and rs["rays_processed"] == 0
    gpu, gs = z.render(C.pointer(s), cam, p)
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k
    if max_depth == 0:
        assert not gpu.any() and gs["rays_processed"] == 0
        assert gs["sampling_loop"] != 4
        assert gs["sampling_loop"] == (3 if bvh else 0)
    else:
        assert gs["sampling_loop"] == ((5 if pool else 4) if bvh else 0)
    if bvh:
        assert gs["schedule_ms"] == 0  # the probe cannot hold the table: tiles in order
    ps = z.RenderParams(**{**p.__dict__, "flags": z.ZRT_FLAG_STATS})
    gpu2, gs2 = z.render(C.pointer(s), cam, ps)
    assert same_bits(gpu, gpu2).all()
    for k in COUNTERS:
        assert gs2[k] == rs[k], k


def test_eight_bit_texels_selected(scenes):
    p = z.RenderParams(8, 8, 1, 2)
    _, gs = z.render(scenes(4), scenes(4).camera, p)
    assert gs["texel_bytes"] == 4  # earthmap from png_image.zig's byte / 255


@pytest.mark.parametrize("world", [1, 3])
def test_schedule_bit_exact(scenes, world):
    """The longest-first tile schedule (probe + device sort, spp >= 128) only
    reorders work: the frame equals the unscheduled one and the oracle's."""
    s = scenes(2)
    p = z.RenderParams(24, 24, 128, 6)
    ref, rs = O.render(s.view, s.camera, p)
    sched = render_partitioned(s, p, world)
    plain = render_partitioned(s, z.RenderParams(24, 24, 128, 6, flags=z.ZRT_FLAG_NO_SCHEDULE), world)
    assert_bit_exact(sched, ref)
    assert_bit_exact(plain, ref)
    gpu, gs = z.render(s, s.camera, p)
    assert gs["schedule_ms"] > 0 and gs["rays_processed"] == rs["rays_processed"]


@pytest.mark.parametrize("rows", [1, 2, 4])
def test_stack_overflow_rows_bit_exact(scenes, rows, monkeypatch):
    """FAST traversal keeps at most ZRT_STACK_LDS_BYTES of its stack in LDS and
    the deeper rows in global memory (deep trees such as scene 6).  Capping the
    LDS part at a few rows (ZRT_STACK_LDS_ROWS) sends most pushes and pops of
    the mesh scenes through the global rows: images and counters unchanged."""
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS", str(rows))
    for idx in (2, 3):
        s = scenes(idx)
        p = z.RenderParams(24, 16, 4, 8)
        ref, rs = O.render(s.view, s.camera, p)
        gpu, gs = z.render(s, s.camera, p)
        assert_bit_exact(gpu, ref)
        for k in COUNTERS:
            assert gs[k] == rs[k], k


# ---- the reference's own full-size run (README.md:39-61): statistical ----------------

def test_c2_matches_reference_showcase_and_readme(golden, scenes):
    """Config C2 (7 spheres, 1000^2 x 1000 spp, depth 30) against the reference's
    own render of it: showcase/7-spheres.png (README.md:39, decoded by libzrt's
    png_image.readFile restatement) and the README's progress counters
    (README.md:50-61).  The reference draws one sequential stream, the GPU one
    per (pixel, sample), so this is the statistical protocol of SURVEY §8c (3):
    channel means within 0.5 %, the 8-bit images within 4 levels on >= 97 % of
    pixels, counters within 10 ppm."""
    import os
    g = golden["reference_tests"]["readme_7spheres"]
    s = scenes(1)
    img, st = z.render(s, s.camera, z.RenderParams(g["width"], g["height"], g["spp"], g["max_depth"]))
    q = np.trunc(np.clip(np.float32(255.999) * img, 0, 255))[::-1]  # png_image.zig:136-140
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    show = np.rint(z.read_png(os.path.join(repo, "assets", "showcase-7-spheres.png"))[::-1].astype(np.float64) * 255)
    np.testing.assert_allclose(q.reshape(-1, 3).mean(0), show.reshape(-1, 3).mean(0), rtol=5e-3)
    d = np.abs(q - show)
    assert (d <= 4).mean() >= 0.97 and d.mean() <= 0.6, (float((d <= 4).mean()), float(d.mean()))
    assert st["samples_processed"] == g["samples"]
    for key, ref in (("rays_processed", g["rays"]), ("reflections", g["reflections"]),
                     ("background_hits", g["background_hits"])):
        assert abs(st[key] - ref) <= 1e-5 * ref, (key, st[key], ref)


# ---- the closest-hit query alone (zrt_trace): BVHNode.hit on random rays ------------

def sphere_scene(spheres):
    """ArrayList(Surface) of spheres, all with Material.black_metal (bvh.zig:244)."""
    from zraytrace_amd import _ffi
    import ctypes as C
    n = len(spheres)
    prims = (_ffi.Prim * n)()
    for i, (x, y, zc, r) in enumerate(spheres):
        prims[i].kind = _ffi.ZRT_PRIM_SPHERE
        prims[i].material = 0
        prims[i].center = _ffi.Vec3(float(x), float(y), float(zc))
        prims[i].radius = float(r)
    texs = (_ffi.Texture * 1)(_ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0, 0, 0), 0.0, 0.0))
    mats = (_ffi.Material * 1)(_ffi.Material(_ffi.ZRT_MAT_METAL, 0, 0.0))
    scene = _ffi.Scene(prims, n, 1, mats, texs, 1, 0, C.cast(None, C.POINTER(_ffi.Image)))
    scene._keep = (prims, mats, texs)
    return scene


TRAVERSALS = [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE, z.ZRT_TRAVERSAL_BINARY]


def assert_same_hits(t_gpu, p_gpu, t_ref, p_ref):
    assert (p_gpu == p_ref).all(), f"{int((p_gpu != p_ref).sum())} rays hit different surfaces"
    assert same_bits(t_gpu, t_ref).all()


def test_trace_reference_bvh_test():
    """bvh.zig:262-291 restated: 3127 random spheres and 2000 random rays from one
    DefaultPrng(42) stream; the reference asserts 10 < hits < 1500.  Here every
    traversal, and the surface list, must return the oracle's closest hit bit
    for bit (t_min 0.001, rayColor's, where the Zig test passes 0.0001)."""
    sph, rays = O.bvh_test_data(z.ZRT_PRNG_XOROSHIRO128, 42, 3127, 2000)
    scene = sphere_scene(sph)
    t_ref, p_ref = O.trace(scene, True, rays[:, :3], rays[:, 3:])
    hits = int((p_ref >= 0).sum())
    assert 10 < hits < 1500, hits
    for trav in TRAVERSALS:
        t, p = z.trace(scene, z.RenderParams(1, 1, 1, 1, traversal=trav), rays[:, :3], rays[:, 3:])
        assert_same_hits(t, p, t_ref, p_ref)
    t_list, p_list = O.trace(scene, False, rays[:, :3], rays[:, 3:])
    t, p = z.trace(scene, z.RenderParams(1, 1, 1, 1, bounded_volume_hierarchy=False), rays[:, :3], rays[:, 3:])
    assert_same_hits(t, p, t_list, p_list)
    # the list and the BVH agree except on exact-t ties between spheres
    assert (p_list == p_ref).mean() > 0.999


@pytest.mark.parametrize("scene_index,rows", [(2, None), (3, None), (0, None), (4, None), (2, "2")])
def test_trace_mesh_rays_bit_exact(scenes, scene_index, rows, monkeypatch):
    """Random rays inside and around the mesh scenes, plus rays aimed exactly at
    triangle vertices and edge midpoints (ties and grazing hits): FAST, BINARY
    and REFERENCE traversal return the oracle's surface and t for every ray.
    rows="2": FAST with a 32-bit stack of 2 LDS rows, so both the traversal and
    its order-hazard replay (the vertex rays have some) run on the global rows."""
    if rows:
        monkeypatch.setenv("ZRT_STACK_LDS_ROWS", rows)
    s = scenes(scene_index)
    origins, dirs = mesh_rays(s, scene_index)
    t_ref, p_ref = O.trace(s.view, True, origins, dirs)
    assert (p_ref >= 0).mean() > 0.3
    for trav in TRAVERSALS:
        t, p = z.trace(s, z.RenderParams(1, 1, 1, 1, traversal=trav), origins, dirs)
        assert_same_hits(t, p, t_ref, p_ref)


def mesh_rays(s, scene_index):
    """test_trace_mesh_rays_bit_exact's rays for a mesh scene: (origins, directions)."""
    from zraytrace_amd import _ffi
    v = s.view.contents
    pr = prim_array(v)
    tri = pr[pr["kind"] == _ffi.ZRT_PRIM_TRIANGLE]
    verts = np.concatenate([tri["a"], tri["b"], tri["c"]]).view(np.float32).reshape(-1, 3)
    lo, hi = verts.min(0), verts.max(0)
    rng = np.random.default_rng(scene_index)
    n = 6000
    o = rng.uniform(lo - (hi - lo), hi + (hi - lo), (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = rng.integers(0, len(tri), 3000)
    a = tri["a"].view(np.float32).reshape(-1, 3)[k]
    b = tri["b"].view(np.float32).reshape(-1, 3)[k]
    c = tri["c"].view(np.float32).reshape(-1, 3)[k]
    targets = np.concatenate([a, (a + b) * np.float32(0.5), (a + b + c) / np.float32(3.0)]).astype(np.float32)
    o2 = np.repeat(np.asarray([s.camera.origin.x, s.camera.origin.y, s.camera.origin.z], np.float32)[None],
                   len(targets), 0) + rng.normal(scale=0.05, size=(len(targets), 3)).astype(np.float32)
    # axis-aligned rays through vertices: slabs with 1/d = inf (NaN bounds) and rays
    # running exactly along box faces and triangle edges (the narrowed test's margin)
    kv = rng.integers(0, len(verts), 2000)
    axis = np.eye(3, dtype=np.float32)[rng.integers(0, 3, 2000)] * rng.choice([-1, 1], (2000, 1)).astype(np.float32)
    o3 = (verts[kv] - axis * np.float32(0.25)).astype(np.float32)
    origins = np.concatenate([o, o2, o3]).astype(np.float32)
    dirs = np.concatenate([d, targets - o2, axis]).astype(np.float32)
    return origins, dirs


def prim_array(v):
    """The scene's zrt_prim array as a numpy structured array (a view)."""
    import ctypes as C
    from zraytrace_amd import _ffi
    dt = np.dtype([("kind", np.uint32), ("material", np.uint32), ("center", np.float32, 3), ("radius", np.float32),
                   ("a", np.float32, 3), ("b", np.float32, 3), ("c", np.float32, 3)])
    assert dt.itemsize == C.sizeof(_ffi.Prim)
    buf = (C.c_uint8 * (dt.itemsize * v.n_prims)).from_address(C.addressof(v.prims.contents))
    return np.frombuffer(buf, dtype=dt)


def test_trace_huge_triangle_det_bit_exact():
    """A triangle with |e1 x e2| ~ 2.6e38: rays through it have det >= 2^126, where
    1/det (triangle.zig:63) is subnormal and the short reciprocal is not exact, so
    the scene takes the IEEE division (KArgs::tri_rcp_fast = 0).  Every traversal
    and the list return the oracle's hits, as on the ordinary triangles beside it."""
    import hazard_rays as H
    big = 8.0e18
    tris = [((-big, 0.0, -big), (-big, 0.0, big), (big, 0.0, -big))]  # e1 x e2 points up (+y)
    rng = np.random.default_rng(5)
    for _ in range(16):  # ordinary triangles just above it, hit from above
        x, zc = rng.uniform(-1, 1, 2)
        y, s = rng.uniform(0.05, 0.25), rng.uniform(0.1, 0.5)
        tris.append(((x, y, zc), (x, y, zc + s), (x + s, y, zc)))
    scene = H.scene_of([], tris)
    n = 4000
    # origins low enough that (o - a) . n stays finite (|n| = 2.56e38)
    o = np.stack([rng.uniform(-1, 1, n), rng.uniform(0.3, 1.2, n), rng.uniform(-1, 1, n)], 1).astype(np.float32)
    d = np.stack([rng.normal(0, 0.3, n), -np.ones(n), rng.normal(0, 0.3, n)], 1).astype(np.float32)
    t_ref, p_ref = O.trace(scene, True, o, d)
    assert (p_ref == 0).sum() > 1000, "rays must reach the huge triangle"
    for trav in TRAVERSALS:
        t, p = z.trace(scene, z.RenderParams(1, 1, 1, 1, traversal=trav), o, d)
        assert_same_hits(t, p, t_ref, p_ref)
    t_list, p_list = O.trace(scene, False, o, d)
    t, p = z.trace(scene, z.RenderParams(1, 1, 1, 1, bounded_volume_hierarchy=False), o, d)
    assert_same_hits(t, p, t_list, p_list)


def test_trace_order_hazard_band_bit_exact():
    """rays whose smallest hit is a sphere hit t* lying
    below its own leaf's loose entry E by a relative (2^-15, 2^-14], with a
    triangle hit in [t*, E] in an earlier DFS leaf, so the reference rejects the
    sphere's leaf and returns the triangle (tests/hazard_rays.py).  Every
    traversal must return the oracle's answer on all of them (and on the 300 000
    rays around them, half of which show some order effect)."""
    import hazard_rays as H
    scene, o, d = H.hazard_scene(1, 300000)
    c = H.classify(O, scene, o, d)
    assert c["hazard"].sum() > 200
    for trav in TRAVERSALS:
        t, p = z.trace(scene, z.RenderParams(1, 1, 1, 1, traversal=trav), o, d)
        hz = c["hazard"]
        assert (p[hz] == c["p_ref"][hz]).all(), f"traversal {trav}: {int((p[hz] != c['p_ref'][hz]).sum())} hazard rays wrong"
        assert_same_hits(t, p, c["t_ref"], c["p_ref"])


def test_reference_box_excess_diagnostic(scenes):
    """The REFERENCE traversal's STATS flavour measures how far the hits the
    reference computes lie outside their own leaf's box (zrt_stats.box_excess_*,
    DESIGN.md §3 "Exactness"): finite, non-negative, identical image."""
    s = scenes(2)
    p = z.RenderParams(64, 64, 4, 20, traversal=z.ZRT_TRAVERSAL_REFERENCE)
    img, _ = z.render(s, s.camera, p)
    p.flags = z.ZRT_FLAG_STATS
    img2, st = z.render(s, s.camera, p)
    assert same_bits(img, img2).all()
    for k in ("box_excess_max_triangle", "box_excess_max_sphere"):
        assert np.isfinite(st[k]) and st[k] >= 0.0, (k, st[k])
    assert st["box_excess_max_triangle"] < 2 ** -12  # the bunny's triangles: far inside FAST's margin


def _grazing_case(scenes, which):
    """(scene view, origins, directions) of tests/grazing_rays.py for a mesh scene
    or for bvh.zig:262-291's 3127 random spheres (which = "spheres")."""
    import grazing_rays as G
    if which == "spheres":
        sph, _ = O.bvh_test_data(z.ZRT_PRNG_XOROSHIRO128, 42, 3127, 1)
        view = sphere_scene(sph)
        keep = view
    else:
        keep = scenes(which)
        view = keep.view
    pr = prim_array(view.contents if hasattr(view, "contents") else view)
    mins, maxs, left, _, _ = O.bvh_build(view)
    o, d = G.grazing_rays(pr, mins, maxs, left, n=6000, seed=7, span=float(np.max(maxs[0] - mins[0])))
    return keep, view, o, d


@pytest.mark.parametrize("which", [2, 3, 0, 4, "spheres"])
def test_trace_grazing_rays_bit_exact(scenes, which):
    """FAST culls a box only when the ray misses it by more
    than the 2^-16 margin, on the assumption that such a box holds no primitive
    the reference hits.  Rays in (or 1-4 ulps beside) the planes of box faces,
    through the triangle vertices and sphere extremes those planes pass through,
    and through leaf box corners and edges (tests/grazing_rays.py): every
    traversal returns the oracle's surface and t bit for bit, the order effects
    among them included (the reference BVH and the list disagree on 1-2 %)."""
    keep, view, o, d = _grazing_case(scenes, which)
    t_ref, p_ref = O.trace(view, True, o, d)
    assert (p_ref >= 0).mean() > 0.5
    for trav in TRAVERSALS:
        t, p = z.trace(keep, z.RenderParams(1, 1, 1, 1, traversal=trav), o, d)
        assert_same_hits(t, p, t_ref, p_ref)


def test_c3_frame_fast_equals_reference_traversal(scenes):
    """the teapot frame (config C3's scene and depth, at 384x384 x
    32 spp) rendered with the FAST traversal, with BINARY and with the reference's
    own traversal (left-first DFS, loose slab test, bvh.zig:187-205) is the same
    frame bit for bit, progress counters included - 8.0 M rays, many of them
    scattered off the teapot at grazing angles."""
    s = scenes(3)
    out = {}
    for trav in TRAVERSALS:
        out[trav] = z.render(s, s.camera, z.RenderParams(384, 384, 32, 20, traversal=trav))
    ref_img, ref_st = out[z.ZRT_TRAVERSAL_REFERENCE]
    assert ref_st["rays_processed"] > 7_000_000
    for trav in (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY):
        img, st = out[trav]
        assert_bit_exact(img, ref_img)
        for k in COUNTERS:
            assert st[k] == ref_st[k], k


@pytest.mark.parametrize("which", [2, 3, 0, 4])
def test_trace_grazing_triangles_bit_exact(scenes, which):
    """rays through points just outside a triangle's vertex, across
    its leaf box's face, nearly parallel to its plane (det 1e-6 .. 1e-3), at gaps
    around the rounded test's measured reach (tests/grazing_tris.py): the
    reference accepts hits whose exact plane crossing lies outside the leaf box by
    up to ~100x FAST's base margins on the teapot.  Without the grazing-triangle
    guard FAST and BINARY got 8 (teapot), 7 (teapot + balls) and 1 (Man) of these
    rays wrong (profiles/r04/r04a); zrt_trace carries the guard, and every
    traversal equals the oracle."""
    import grazing_tris as G
    s = scenes(which)
    pr = prim_array(s.view.contents)
    mins, maxs, left, right, _ = O.bvh_build(s.view)
    o, d = G.grazing_triangle_rays(pr, mins, maxs, left, right, n=20000, seed=1, span=G.scene_span(pr))
    p_ref, bad = _trace_all(s.view, o, d, keep=s)
    assert (p_ref >= 0).mean() > 0.5
    assert not bad, f"rays differing from the oracle, per traversal: {bad}"


def test_trace_grazing_triangles_c5_substitute(scenes):
    """The grazing-triangle set (tests/grazing_tris.py) on scene 6, the 1.6 M-triangle
    subdivided teapot that stands in for C5 (VERDICT r03 #1 names it): its leaves
    are tiny, so near-plane hits land close to many leaf faces.  The reference BVH
    comes from the GPU build (zrt_bvh_build_device, equal to the host build on
    this scene in test_device_bvh_c5_substitute); FAST and BINARY must equal the
    REFERENCE traversal on all 4000 rays, and the REFERENCE traversal the oracle on
    the first 400 (the oracle's own BVH build of this mesh takes most of a minute)."""
    import grazing_tris as G
    s = scenes(6)
    pr = prim_array(s.view.contents)
    mins, maxs, left, right, _ = z.bvh_build_device(s)
    o, d = G.grazing_triangle_rays(pr, mins, maxs, left, right, n=4000, seed=2, span=G.scene_span(pr))
    res = {trav: z.trace(s, z.RenderParams(1, 1, 1, 1, traversal=trav), o, d) for trav in TRAVERSALS}
    t_ref, p_ref = res[z.ZRT_TRAVERSAL_REFERENCE]
    assert (p_ref >= 0).mean() > 0.5
    bad = {trav: int(((p != p_ref) | ~same_bits(t, t_ref)).sum()) for trav, (t, p) in res.items()}
    assert not any(bad.values()), f"rays differing from the REFERENCE traversal: {bad}"
    t_o, p_o = O.trace(s.view, True, o[:400], d[:400])
    assert np.array_equal(p_o, p_ref[:400]) and same_bits(t_o, t_ref[:400]).all()


@pytest.mark.parametrize("which", [2, 3, 0, 4])
def test_trace_grazing_triangles_unguarded_recorded(scenes, which, monkeypatch):
    """the same grazing-triangle rays traced WITHOUT the guard
    (ZRT_DEBUG_NO_GUARD: the traversal the default, unguarded render kernels run).
    The count of rays whose answer differs from the oracle is recorded (printed;
    round 3's kernel: teapot 8, teapot + balls 7, Man 1 of 20 000).  What is
    asserted is the tolerance the unguarded default claims: a flip changes one
    sample of one pixel, and such rays are at most 1 in 1000 of this deliberately
    adversarial set; the guarded traversal (the test above) has none."""
    import grazing_tris as G
    s = scenes(which)
    pr = prim_array(s.view.contents)
    mins, maxs, left, right, _ = O.bvh_build(s.view)
    o, d = G.grazing_triangle_rays(pr, mins, maxs, left, right, n=20000, seed=1, span=G.scene_span(pr))
    monkeypatch.setenv("ZRT_DEBUG_NO_GUARD", "1")
    _, bad = _trace_all(s.view, o, d, keep=s)
    # the counts are persisted, not printed: every run
    # writes them to gpurun_out/records/grazing_unguarded.json (merged back from the GPU
    # box; committed as profiles/grazing_unguarded.json), and a count above the
    # committed one for this scene fails - the gap may shrink, never grow unnoticed
    names = {z.ZRT_TRAVERSAL_FAST: "fast", z.ZRT_TRAVERSAL_BINARY: "binary", z.ZRT_TRAVERSAL_REFERENCE: "reference"}
    counts = {names.get(k, str(k)): int(v) for k, v in bad.items()}
    rec_dir = os.path.join(REPO, "gpurun_out", "records")
    os.makedirs(rec_dir, exist_ok=True)
    rec_path = os.path.join(rec_dir, "grazing_unguarded.json")
    rec = json.load(open(rec_path)) if os.path.exists(rec_path) else {}
    rec[f"scene{which}"] = {"rays": int(len(o)), "differing_from_oracle": counts, "build_id": z.build_id()}
    with open(rec_path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    committed = os.path.join(REPO, "profiles", "grazing_unguarded.json")
    if os.path.exists(committed):
        entry = json.load(open(committed)).get(f"scene{which}")
        if entry is not None:  # (a traversal absent from the record had no differing ray)
            ref = entry.get("differing_from_oracle", {})
            for trav, v in counts.items():
                assert v <= ref.get(trav, 0), f"scene {which} {trav}: {v} differing rays, committed {ref.get(trav, 0)}"
    assert counts.get("reference", 0) == 0  # (the reference's own traversal has no guard to lose)
    assert all(v <= 20 for v in counts.values()), counts


@pytest.mark.parametrize("scene_index,dims", [(4, (128, 128, 8)), (6, (96, 96, 8))], ids=["teapot-balls", "c5-mesh"])
def test_unguarded_render_equals_reference_traversal(scenes, scene_index, dims):
    """the default (unguarded) FAST render on the meshes the
    guard exists for - scene 4 (teapot + ring of spheres) and scene 6 (the 1.6 M
    triangle C5 mesh, path-pool loop) - against the REFERENCE traversal (the
    reference's left-first DFS with its loose slab test, bvh.zig:187-205) on the
    same frame, > 10^5 rays at depth 20: bit-identical, counters included."""
    s = scenes(scene_index)
    w, h, spp = dims
    fast_img, fast_st = z.render(s, s.camera, z.RenderParams(w, h, spp, 20))
    ref_img, ref_st = z.render(s, s.camera, z.RenderParams(w, h, spp, 20, traversal=z.ZRT_TRAVERSAL_REFERENCE))
    assert ref_st["rays_processed"] > 100_000
    assert fast_st["guard"] == 0.0
    diff = int((~(fast_img.view(np.uint32) == ref_img.view(np.uint32))).any(axis=2).sum())
    assert diff == 0, f"{diff} pixels differ from the REFERENCE traversal's frame"
    for k in COUNTERS:
        assert fast_st[k] == ref_st[k], k


@pytest.mark.parametrize("scene_index", [3, 4])
def test_render_with_grazing_guard_bit_exact(scenes, scene_index):
    """ZRT_FLAG_GUARD: the render carries the grazing-triangle guard (in the
    path-pool loop): the frame, its counters and per-scanline counters equal the
    oracle's, and zrt_stats reports the guard's coefficient."""
    s = scenes(scene_index)
    p = z.RenderParams(40, 32, 6, 20, sample_chunk=4, flags=z.ZRT_FLAG_GUARD)
    gpu, gs, rows = z.render_progress(s, s.camera, p)
    ref, rs, rrows = O.render_scanlines(s.view, s.camera, z.RenderParams(40, 32, 6, 20, sample_chunk=4))
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k
    np.testing.assert_array_equal(rows, rrows)
    assert gs["guard"] > 0.0 and gs["sampling_loop"] == 5
    _, g0 = z.render(s, s.camera, z.RenderParams(16, 16, 1, 4))
    assert g0["guard"] == 0.0  # (off by default)


# ---- adversarial cases against FAST's exactness argument ----

def _trace_all(scene, o, d, keep=None):
    t_ref, p_ref = O.trace(scene, True, o, d)
    bad = {}
    for trav in TRAVERSALS:
        t, p = z.trace(keep or scene, z.RenderParams(1, 1, 1, 1, traversal=trav), o, d)
        wrong = (p != p_ref) | ~same_bits(t, t_ref)
        if wrong.any():
            bad[trav] = int(wrong.sum())
    return p_ref, bad


@pytest.mark.parametrize("seed", [0, 1])
def test_trace_near_miss_spheres_bit_exact(seed):
    """Rays just outside small, distant spheres (tests/adversarial_rays.py): the
    rounded disc of sphere.zig:31-41 accepts thousands of them although they miss
    the sphere (and its box), and some run past facing triangles placed just in
    front of tangent points.  Every traversal returns the oracle's answer."""
    import adversarial_rays as A
    scene, o, d = A.near_miss_scene(seed)
    p_ref, bad = _trace_all(scene, o, d)
    assert (p_ref >= 0).sum() > 10000
    assert not bad, f"rays differing from the oracle, per traversal: {bad}"


@pytest.mark.parametrize("which,scale,translate", [(2, 1.0, 1e3), (2, 1.0, 1e4), (2, 1e-3, 0.0), (2, 1e3, 0.0),
                                                   (3, 1.0, 1e3), (3, 1.0, 1e4), (3, 1e-3, 0.0), (3, 1e3, 0.0)])
def test_trace_transformed_scenes_bit_exact(scenes, which, scale, translate):
    """the bunny and teapot scenes (ground sphere included)
    translated by 10^3 / 10^4 and scaled by 10^-3 / 10^3, with the grazing rays of
    tests/grazing_rays.py and random rays: every traversal equals the oracle."""
    import adversarial_rays as A
    pr = A.prim_array(scenes(which).view.contents)
    scene, o, d = A.transformed_case(O, pr, scale, translate, seed=which)
    p_ref, bad = _trace_all(scene, o, d)
    assert (p_ref >= 0).mean() > 0.2
    assert not bad, f"rays differing from the oracle, per traversal: {bad}"


@pytest.mark.parametrize("translate", [1e3, 1e4])
def test_trace_far_spheres_bit_exact(translate):
    """bvh.zig:262-291's spheres and rays moved 10^3 / 10^4 from the origin, plus
    grazing rays: every traversal equals the oracle."""
    import adversarial_rays as A
    scene, o, d = A.far_spheres_case(O, translate)
    p_ref, bad = _trace_all(scene, o, d)
    assert (p_ref >= 0).sum() > 300
    assert not bad, f"rays differing from the oracle, per traversal: {bad}"


# ---- per-axis margins for nearly axis-parallel rays ----

def _fast(scene, o, d, keep=None):
    t_ref, p_ref = O.trace(scene, True, o, d)
    t, p = z.trace(keep or scene, z.RenderParams(1, 1, 1, 1, traversal=z.ZRT_TRAVERSAL_FAST), o, d)
    return int(((p != p_ref) | ~same_bits(t, t_ref)).sum()), p_ref


def _near_parallel_rays(lo, hi, n, seed):
    """Rays through random points of the box [lo, hi] whose direction has one
    component 2^-40 .. 2^-6 (either sign) or exactly 0: max_k |1/d_k| from 64 to
    inf, the rays the t-space margins turned the narrowed cull off for."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    k = rng.integers(0, 3, n)
    tiny = (2.0 ** rng.uniform(-40, -6, n) * rng.choice([-1, 1], n)).astype(np.float32)
    tiny[rng.random(n) < 0.1] = 0.0
    d[np.arange(n), k] = tiny
    o = (p - d / np.linalg.norm(d, axis=1, keepdims=True) * np.float32(rng.uniform(0.2, 2.0))
         * np.float32(np.max(hi - lo))).astype(np.float32)
    return o, d


@pytest.mark.parametrize("which", [2, 3, "spheres", "bunny1e4"])
def test_trace_per_axis_margins_every_wave_bit_exact(scenes, which, monkeypatch):
    """The per-axis widening of wide_iter (paxis_slot) taken by EVERY wave
    (ZRT_PAXIS_M=0) on the grazing rays of tests/grazing_rays.py, on nearly
    axis-parallel rays and (bunny1e4) on the bunny scene moved 10^4 from the
    origin: FAST equals the oracle bit for bit.  At the default threshold the
    same rays take it only in waves with such a lane (the other trace tests)."""
    monkeypatch.setenv("ZRT_PAXIS_M", "0")
    if which == "bunny1e4":
        import adversarial_rays as A
        pr = A.prim_array(scenes(2).view.contents)
        scene, o, d = A.transformed_case(O, pr, 1.0, 1e4, seed=2)
        keep = None
    else:
        keep, scene, o, d = _grazing_case(scenes, which)
    prv = prim_array(scene.contents if hasattr(scene, "contents") else scene)
    from zraytrace_amd import _ffi
    tri = prv[prv["kind"] == _ffi.ZRT_PRIM_TRIANGLE]
    pts = (np.concatenate([tri["a"], tri["b"], tri["c"]]) if len(tri) else prv["center"]).reshape(-1, 3)
    assert np.isfinite(pts).all()
    o2, d2 = _near_parallel_rays(pts.min(0), pts.max(0), 6000, seed=11)
    o = np.concatenate([o, o2]).astype(np.float32)
    d = np.concatenate([d, d2]).astype(np.float32)
    wrong, p_ref = _fast(scene, o, d, keep)
    assert (p_ref >= 0).mean() > 0.2
    assert wrong == 0, f"{wrong} rays differ from the oracle"


@pytest.mark.parametrize("loop", ["wavefront", "pool"])
def test_render_per_axis_margins_every_wave(scenes, loop, monkeypatch):
    """The deep-tree loops with the per-axis margins in every wave
    (ZRT_PAXIS_M=0): the teapot frame equals the oracle's bit for bit."""
    set_loop(monkeypatch, loop)
    monkeypatch.setenv("ZRT_PAXIS_M", "0")
    s = scenes(3)
    p = z.RenderParams(48, 40, 6, 20, sample_chunk=4)
    gpu, gs = z.render(s, s.camera, p)
    ref, rs = O.render(s.view, s.camera, p)
    assert_bit_exact(gpu, ref)
    for k in COUNTERS:
        assert gs[k] == rs[k], k

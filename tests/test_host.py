"""Host-side tests of the product library (no kernel launches; CPU only).

* libzrt.so loads and exports every symbol include/zrt.h declares;
* scene ingestion (scenes.zig / obj_reader.zig restatement) matches the
  reference's model statistics;
* the product BVH (zrt_bvh_build) is the oracle's tree, node for node;
* the C ABI reports the reference's error cases.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    src = open(os.path.join(REPO, "include", "zrt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(zrt_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _ffi.load()
    syms = header_symbols()
    assert len(syms) >= 18
    for name in syms:
        assert hasattr(lib, name), name
    # the ctypes table covers the header exactly
    assert sorted(n for n, _, _ in _ffi.SIGNATURES) == syms


def test_abi_version_and_struct_sizes():
    lib = _ffi.load()
    assert lib.zrt_abi_version() == 2 == _ffi.ABI_VERSION
    assert b"gfx950" in lib.zrt_build_info()
    assert C.sizeof(_ffi.Prim) == 60 and C.sizeof(_ffi.Camera) == 48
    assert C.sizeof(_ffi.Params) == 64 and C.sizeof(_ffi.BvhNode) == 32


@pytest.mark.parametrize("index,n_prims", [(0, 1 + 3933), (1, 7), (2, 1 + 4968), (3, 1 + 6320), (4, 3 + 6320)])
def test_scene_sizes(scenes, index, n_prims):
    """scenes.zig + obj_reader.zig: Man 1962 quads + 6 tris + 1 pentagon -> 3933
    triangles; bunny 4968; teapot 6320 (SURVEY §2 models row)."""
    assert scenes(index).n_prims == n_prims


def test_scene_errors():
    with pytest.raises(z.ZrtError) as e:
        z.load_scene(9)
    assert e.value.code == _ffi.ZRT_E_INVALID and "UnkownSceneIndex" in str(e.value)
    with pytest.raises(z.ZrtError) as e:
        z.load_scene(5)  # goat: models/high_poly_goat.obj is not shipped
    assert e.value.code == _ffi.ZRT_E_IO


def test_obj_reader_fan_order(tmp_path):
    """obj_reader.zig:66-111: 3..6-gons fan as 0,1,2 | 2,3,0 | 3,4,0 | 4,5,0;
    'v//vn' and 'v/vt/vn' forms; CRLF lines; >6 vertices is an error."""
    p = tmp_path / "m.obj"
    p.write_bytes(b"# c\r\nv 0 0 0\r\nv 1 0 0\r\nv 1 1 0\r\nv 0 1 0\r\nv 0 2 0\nv 3 3 3\n"
                  b"vn 0 0 1\nf 1//1 2//1 3//1 4//1\nf 1/1/1 2/2/2 3/3/3 4/4/4 5/5/5 6/6/6\nf 1 2 3\n")
    prims = C.POINTER(_ffi.Prim)()
    n = C.c_uint32()
    _ffi.check(_ffi.load().zrt_obj_read(str(p).encode(), 7, C.byref(prims), C.byref(n)))
    tris = [(tuple((prims[i].a.x, prims[i].a.y)), tuple((prims[i].b.x, prims[i].b.y)),
             tuple((prims[i].c.x, prims[i].c.y))) for i in range(n.value)]
    _ffi.load().zrt_free(C.cast(prims, C.c_void_p))
    assert n.value == 2 + 4 + 1
    assert tris[0] == ((0, 0), (1, 0), (1, 1)) and tris[1] == ((1, 1), (0, 1), (0, 0))
    assert tris[3] == ((1, 1), (0, 1), (0, 0)) and tris[4] == ((0, 1), (0, 2), (0, 0))
    assert tris[5] == ((0, 2), (3, 3), (0, 0))
    bad = tmp_path / "bad.obj"
    bad.write_text("v 0 0 0\nv 1 0 0\nf 1 2\n")
    rc = _ffi.load().zrt_obj_read(str(bad).encode(), 0, C.byref(prims), C.byref(n))
    assert rc == _ffi.ZRT_E_PARSE


@pytest.mark.parametrize("index", [0, 1, 2, 3, 4])
def test_bvh_matches_oracle(scenes, index):
    """bvh.zig:62-185: the product's flat BVH equals the oracle's pointer tree
    (same topology, same boxes bit for bit, same leaf order, same depth)."""
    s = scenes(index)
    a = z.bvh_build(s)
    b = O.bvh_build(s.view)
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
    assert a[4] == b[4]


def test_bvh_depths(scenes):
    """SURVEY §3.2 probe: bunny 6531 nodes / depth 23, teapot 7573 / 23."""
    mins, _, _, _, depth = z.bvh_build(scenes(2))
    assert (len(mins), depth) == (6531, 23)
    mins, _, _, _, depth = z.bvh_build(scenes(3))
    assert (len(mins), depth) == (7573, 23)


def test_camera_init_matches_oracle():
    got = z.camera_init((0, 0, -0.5), (0, 0, 1), (0, 1, 0), 45.0, 1.0)
    want = O.camera_init((0, 0, -0.5), (0, 0, 1), (0, 1, 0), 45.0, 1.0)
    assert bytes(got) == bytes(want)


def test_param_validation_without_device(scenes):
    """Reference error behaviour maps to ZRT_E_*; with no GPU the HIP path
    reports ZRT_E_NODEVICE instead of silently falling back."""
    s = scenes(1)
    cam = s.camera
    with pytest.raises(z.ZrtError) as e:
        z.render(s, cam, z.RenderParams(8, 16, 1, 5))  # height > width (raytrace.zig:168)
    assert e.value.code == _ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:
        z.render(s, cam, z.RenderParams(8, 8, 1, 5, rng_mode=z.ZRT_RNG_REFERENCE_STREAM))
    assert e.value.code == _ffi.ZRT_E_UNSUPPORTED
    with pytest.raises(z.ZrtError) as e:
        z.render(s, cam, z.RenderParams(8, 8, 70000, 5))
    assert e.value.code == _ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:  # zrt_trace: unknown traversal, checked before the device
        z.trace(s, z.RenderParams(1, 1, 1, 1, traversal=7), [[0, 0, 0]], [[0, 0, 1]])
    assert e.value.code == _ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:  # zrt_render_multi: empty device list
        z.render_multi(s, cam, z.RenderParams(8, 8, 1, 5), [])
    assert e.value.code == _ffi.ZRT_E_INVALID
    import torch
    if not torch.cuda.is_available():
        for call in (lambda: z.render(s, cam, z.RenderParams(8, 8, 1, 5)),
                     lambda: z.render_multi(s, cam, z.RenderParams(8, 8, 1, 5), [0, 1]),
                     lambda: z.trace(s, z.RenderParams(1, 1, 1, 1), [[0, 0, 0]], [[0, 0, 1]])):
            with pytest.raises(z.ZrtError) as e:
                call()
            assert e.value.code == _ffi.ZRT_E_NODEVICE


def test_debug_compact_refusals():
    """zrt_debug_compact checks its list on the host, before any device is asked for: the
    kernel indexes tile_done with the entries.  A null pointer, an empty list, an entry at or
    past n_tiles: ZRT_E_INVALID; a good list with no GPU: ZRT_E_NODEVICE."""
    u32p = C.POINTER(C.c_uint32)
    lst, done, out, count = (C.c_uint32 * 3)(0, 2, 1), (C.c_uint32 * 3)(), (C.c_uint32 * 3)(), C.c_uint32()
    f = z.lib().zrt_debug_compact
    for args in ((None, 3, done, 3, out, C.byref(count), 0), (lst, 3, None, 3, out, C.byref(count), 0),
                 (lst, 3, done, 3, None, C.byref(count), 0), (lst, 3, done, 3, out, None, 0),
                 (lst, 0, done, 3, out, C.byref(count), 0), (lst, 3, done, 2, out, C.byref(count), 0)):
        assert f(*args) == _ffi.ZRT_E_INVALID, args
    for bad in ([], [3], [0, 1, 2 ** 32 - 1]):
        with pytest.raises(z.ZrtError) as e:
            z.debug_compact(bad, [0, 0, 0])
        assert e.value.code == _ffi.ZRT_E_INVALID, bad
    assert C.cast(out, u32p)[0] == 0  # (refused before anything is written)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(z.ZrtError) as e:
            z.debug_compact([0, 2, 1], [0, 0, 0])
        assert e.value.code == _ffi.ZRT_E_NODEVICE


def test_tree_layout_mismatch_is_refused(scenes, monkeypatch):
    """a wide tree whose encoding is not the one the kernels
    decode (accel_build.hpp kLayout*, render.hip kKernelLayout) is refused with
    ZRT_E_UNSUPPORTED before anything is launched - here on CPU, where the check
    runs before the device check.  (The kernels repeat the check on the device:
    kErrLayout.)"""
    s = scenes(2)
    monkeypatch.setenv("ZRT_DEBUG_TREE_LAYOUT", "1")  # flips the sphere-slot bit of the recorded layout
    for call in (lambda: z.render(s, s.camera, z.RenderParams(8, 8, 1, 5)),
                 lambda: z.RenderContext(s, z.RenderParams(8, 8, 1, 5))):
        with pytest.raises(z.ZrtError) as e:
            call()
        assert e.value.code == _ffi.ZRT_E_UNSUPPORTED and "layout" in str(e.value)
    monkeypatch.delenv("ZRT_DEBUG_TREE_LAYOUT")
    import torch
    if not torch.cuda.is_available():  # the matching layout passes on to the device check
        with pytest.raises(z.ZrtError) as e:
            z.render(s, s.camera, z.RenderParams(8, 8, 1, 5))
        assert e.value.code == _ffi.ZRT_E_NODEVICE


def test_oracle_counters_readme_rays_per_sample(scenes):
    """README.md:50-61: scene 1 at depth 30 spends 2.1446 rays per sample; the
    oracle (reference stream) lands within 2% on a 48x48x8 sample."""
    s = scenes(1)
    img, st = O.render(s.view, s.camera, z.RenderParams(48, 48, 8, 30, rng_mode=z.ZRT_RNG_REFERENCE_STREAM))
    rps = st["rays_processed"] / st["samples_processed"]
    assert abs(rps - 2144645362 / 1e9) / 2.1446 < 0.02
    assert st["pixels_processed"] == 48 * 48 and st["samples_processed"] == 48 * 48 * 8
    # counters are consistent: samples + reflections = rays + depth hits
    assert st["samples_processed"] + st["reflections"] == st["rays_processed"] + st["recursion_depth_hits"]


def test_oracle_counter_mode_is_row_separable(scenes):
    """In counter mode every pixel has its own streams: rendering rows [8, 16)
    alone gives the same pixels as the full frame."""
    s = scenes(1)
    p = z.RenderParams(16, 16, 2, 10)
    full, _ = O.render(s.view, s.camera, p)
    part, _ = O.render(s.view, s.camera, p, rows=(8, 16))
    np.testing.assert_array_equal(full[8:16], part[8:16])


def _synthetic_scene(n, seed):
    """n primitives on a coarse lattice (many equal midpoints, +-0 coordinates,
    spheres and triangles mixed): the cases where a sort's tie order shows."""
    rng = np.random.default_rng(seed)
    prims = (_ffi.Prim * n)()
    lattice = np.array([-1.0, -0.5, -0.0, 0.0, 0.5, 1.0], np.float32)
    for i in range(n):
        p = prims[i]
        if rng.random() < 0.3:
            p.kind = _ffi.ZRT_PRIM_SPHERE
            p.center = _ffi.Vec3(*rng.choice(lattice, 3))
            p.radius = float(rng.choice([0.25, 0.5]))
        else:
            p.kind = _ffi.ZRT_PRIM_TRIANGLE
            base = rng.choice(lattice, 3)
            p.a = _ffi.Vec3(*base)
            p.b = _ffi.Vec3(*(base + rng.choice(lattice, 3)))
            p.c = _ffi.Vec3(*(base + rng.choice(lattice, 3)))
    mats = (_ffi.Material * 1)(_ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 0, 0.0))
    texs = (_ffi.Texture * 1)(_ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0.5, 0.5, 0.5), 0.0, 0.0))
    scene = _ffi.Scene(prims, n, 1, mats, texs, 1, 0, None)
    scene._keep = (prims, mats, texs)
    return scene


@pytest.mark.parametrize("n,seed", [(50, 1), (3000, 2), (20000, 3)])
def test_bvh_ties_match_oracle(n, seed):
    """The radix-sorted build (one sort per axis, stable LSD radix, -0 == +0)
    equals the oracle's comparison-sort restatement of bvh.zig node for node
    on inputs full of equal keys and signed zeros."""
    s = _synthetic_scene(n, seed)
    a = z.bvh_build(C.pointer(s))
    b = O.bvh_build(C.pointer(s))
    for x, y in zip(a[:4], b[:4]):
        np.testing.assert_array_equal(x, y)
    assert a[4] == b[4]


@pytest.mark.parametrize("index", [1, 6])
def test_binary_scene_round_trip(tmp_path, index):
    """zrt_scene_write / zrt_scene_read: every array of the flat scene, the
    images and the camera come back byte for byte (the 7-spheres scene with its
    earthmap texture; the 1.6 M-triangle C5 substitute), and the BVH built from
    it is the same tree."""
    import time
    t0 = time.time()
    s = z.load_scene(index)
    t_load = time.time() - t0
    path = str(tmp_path / f"scene{index}.zrts")
    s.write(path)
    t0 = time.time()
    r = z.LoadedScene.read(path)
    t_read = time.time() - t0
    a, b = s.view.contents, r.view.contents
    assert bytes(s.camera) == bytes(r.camera)
    for name, typ in (("prims", _ffi.Prim), ("materials", _ffi.Material), ("textures", _ffi.Texture)):
        n = getattr(a, "n_" + name)
        assert getattr(b, "n_" + name) == n
        size = C.sizeof(typ) * n
        assert C.string_at(getattr(a, name), size) == C.string_at(getattr(b, name), size), name
    assert a.n_images == b.n_images
    for i in range(a.n_images):
        ia, ib = a.images[i], b.images[i]
        assert (ia.width, ia.height) == (ib.width, ib.height)
        n = 12 * ia.width * ia.height
        assert C.string_at(ia.pixels, n) == C.string_at(ib.pixels, n)
    if index == 1:
        ta = z.bvh_build(s)
        tb = z.bvh_build(r)
        for x, y in zip(ta[:4], tb[:4]):
            np.testing.assert_array_equal(x, y)
    print(f"scene {index}: built {t_load:.3f} s, read back {t_read:.3f} s")


def test_binary_scene_rejects(tmp_path):
    bad = tmp_path / "bad.zrts"
    bad.write_bytes(b"NOPE" + bytes(64))
    with pytest.raises(z.ZrtError) as e:
        z.LoadedScene.read(str(bad))
    assert e.value.code == _ffi.ZRT_E_PARSE
    s = z.load_scene(1)
    good = tmp_path / "good.zrts"
    s.write(str(good))
    data = good.read_bytes()
    (tmp_path / "cut.zrts").write_bytes(data[:-100])
    # header counts from the file are checked against its size before
    # anything is allocated (2^32 - 1 primitives would ask for 240 GB)
    huge = bytearray(data)
    huge[4 + 4 * 4: 4 + 4 * 5] = (0xFFFFFFFF).to_bytes(4, "little")  # head[4] = n_prims
    (tmp_path / "huge.zrts").write_bytes(bytes(huge))
    for name in ("cut.zrts", "huge.zrts"):
        with pytest.raises(z.ZrtError) as e:
            z.LoadedScene.read(str(tmp_path / name))
        assert e.value.code == _ffi.ZRT_E_PARSE, name
    with pytest.raises(z.ZrtError) as e:
        z.LoadedScene.read(str(tmp_path / "missing.zrts"))
    assert e.value.code == _ffi.ZRT_E_IO


def test_stats_struct_matches_header():
    """zraytrace_amd._ffi.Stats lists zrt_stats's fields (include/zrt.h) in order, so
    a field added to the C struct cannot shift the ctypes layout unnoticed."""
    import re
    with open(os.path.join(REPO, "include", "zrt.h")) as f:
        h = f.read()
    body = h[h.index("typedef struct zrt_stats {"):h.index("} zrt_stats;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\b(?:u?int(?:32|64)_t|float|double)\s+(\w+)\s*;", body)
    assert names == [n for n, _ in _ffi.Stats._fields_]



def test_u8_texel_values_by_short_division():
    """render.hip att_value decodes an 8-bit texel k as dev::div_known(k, 255,
    RN(1/255)) - q = RN(k y), r = fma(-q, 255, k), RN(r y + q) - instead of a table of
    the reference's k / 255.0f (png_image.zig:88).  Checked here with exact rational
    arithmetic for every k: the same f32 bits."""
    from fractions import Fraction as F

    def rn32(x):
        f = np.float32(float(x))
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        return min(cands, key=lambda c: (abs(F(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))

    b = np.float32(255.0)
    y = np.float32(1.0) / b
    for k in range(256):
        a = np.float32(k)
        q = rn32(F(float(a)) * F(float(y)))
        r = rn32(F(float(a)) - F(float(q)) * F(float(b)))
        got = rn32(F(float(r)) * F(float(y)) + F(float(q)))
        assert np.float32(got).view(np.uint32) == (np.float32(k) / b).view(np.uint32), k


@pytest.mark.parametrize("index", [0, 1, 2, 3, 4])
def test_lds_plans_disjoint(scenes, index):
    """every LDS layout the launch code plans for the scene -
    list, binary, reference, lockstep / wavefront / path-pool FAST loops, 16- and
    32-bit stacks, both PRNGs, max depths 0..50 - keeps its regions (stack rows,
    top wide nodes, pool queues, the lockstep loop's parked lane state, attenuation
    rows, materials) disjoint, inside the plan and float4-aligned, and the lockstep
    plan inside its 6-block share (planner.cpp check_plan).  No device needed."""
    n = z.debug_lds_plans(scenes(index))
    # modes 0-2 one loop each, mode 3 lockstep / wavefront / pool (full nodes, and compressed
    # ones where the scene has a tree: their real top levels); x stk16 x prng x depth
    comp = 0 if index == 1 else 1
    # + the FAST loops' 16-bit plans with their LDS stack rows capped at 1, 2 and 4
    # (ZRT_STACK_LDS_ROWS16), x prng x depth
    assert n == (1 + 1 + 1 + 1 + 1 + 1 + comp) * 2 * 2 * 6 + (1 + 1 + 1 + comp) * 3 * 2 * 6


@pytest.mark.parametrize("index", [0, 2, 3, 4])
def test_shared_buffer_sizing_covers_every_launch(scenes, index):
    """the global rows a FAST frame's launches share - the
    attenuation rows past the LDS ones and the stack rows past the LDS ones - are
    sized (zrt_render, schedule_tiles) to cover the render launch AND its scheduling
    probe, for every loop x stack width x PRNG x node format x depth x grid
    (planner.cpp buffer_need / check_buffers, the same check that guards each launch).
    The sizing before commit 4072f5f (the probe reused the render's attenuation rows
    without growing them) must fail where the render keeps more LDS rows than the
    probe's 4: the wavefront loop's 12 - the round-5 GPU fault of ZRT_WF=1 on C3."""
    s = scenes(index)
    n = z.debug_buffer_plans(s)
    # lockstep, wavefront, pool (+ compressed) x stk16 x prng x depth x grid, + the 16-bit
    # stacks with their LDS rows capped at 1, 2 and 4 (ZRT_STACK_LDS_ROWS16)
    assert n >= 3 * 2 * 2 * 9 * 3 + 3 * 3 * 2 * 9 * 3
    with pytest.raises(z.ZrtError, match="scheduling probe: needs .* attenuation-row entries.*loop 1"):
        z.debug_buffer_plans(s, legacy=True)


TRAVERSALS = (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE)
PRNGS = (z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256)
NEEDS_DEPTH = (4, 5, 7, 8, 9)  # the wavefront and path-pool kernels: written for max_depth >= 1
LOOP_KNOBS = ("ZRT_WF", "ZRT_POOL", "ZRT_LIST_LANES")


def _plan_scene(scenes, which):
    if which == "many-materials":
        import many_materials as M
        s = M.many_materials_scene()
        return s, C.pointer(s)
    s = scenes(which)
    return s, s.view


def _check_plan(d, depth, where):
    """The invariants of one launch decision (zrt_debug_launch_plan)."""
    assert d["sampling_loop"] == (5 if d["kmode"] in (7, 8, 9) else d["kmode"]), where
    # 1. a loop whose kernel assumes max_depth >= 1 is chosen only there
    if d["kmode"] in NEEDS_DEPTH:
        assert depth >= 1, where
    # 2. the loops that read the material table from LDS only have it there, or shade nothing
    if d["kmode"] in (3, 6):
        assert d["mats_in_lds"] or depth == 0, where
    # 3. every attenuation row a kernel can index is allocated: rows 0 .. max_depth-2 are
    #    pushed, the first att_rows of them live in LDS
    assert d["att_rows_per_path"] >= max(1, depth - 1 - d["att_rows"]), where
    # 4. the stack rows past the LDS ones are allocated, at the stack's width
    assert d["stack_rows"] <= max(d["stack_depth"], 1), where
    ovf_rows = max(0, d["stack_depth"] - d["stack_rows"])
    assert d["ovf_bytes_per_lane"] >= ovf_rows * (2 if d["stk16"] else 4), where
    assert d["lds_bytes"] <= 160 << 10, where


@pytest.mark.parametrize("which", [0, 1, 2, 3, 4, "many-materials"])
def test_launch_plan_invariants(scenes, which, monkeypatch):
    """The launch decision of zrt_ctx_render_tiles (planner.cpp plan_launch, reported
    with no device by zrt_debug_launch_plan) over traversal x max_depth x PRNG x the
    loop knobs (ZRT_WF, ZRT_POOL, ZRT_LIST_LANES: unset, 0, 1) x ZRT_FLAG_GUARD x the
    16-bit stack-row cap (ZRT_STACK_LDS_ROWS16): the invariants of _check_plan.

    The knobs are crossed in full on the many-materials grid, where the material-table
    fallback is taken (and which flattens in a millisecond).  The reference scenes
    flatten in 10 - 40 ms a call: there ZRT_WF x ZRT_POOL are crossed for FAST (the
    only traversal that reads them) with ZRT_LIST_LANES varied alone - on the seven
    spheres, a list scene, ZRT_LIST_LANES is crossed and the other two varied alone -
    and the other traversals run with every knob unset and with every knob set."""
    keep, view = _plan_scene(scenes, which)
    vals = (None, "0", "1")
    unset = dict.fromkeys(LOOP_KNOBS)
    if which == "many-materials":
        fast = [dict(zip(LOOP_KNOBS, (a, b, c))) for a in vals for b in vals for c in vals]
        other = fast
    elif which == 1:
        fast = [{**unset, "ZRT_LIST_LANES": c} for c in vals] + [{**unset, "ZRT_WF": "1"}, {**unset, "ZRT_POOL": "1"}]
        other = [unset, {"ZRT_WF": "1", "ZRT_POOL": "1", "ZRT_LIST_LANES": "0"}]
    else:
        fast = [{**unset, "ZRT_WF": a, "ZRT_POOL": b} for a in vals for b in vals]
        fast += [{**unset, "ZRT_LIST_LANES": c} for c in ("0", "1")]
        other = [unset, {"ZRT_WF": "1", "ZRT_POOL": "1", "ZRT_LIST_LANES": "0"}]
    n = 0
    for trav in TRAVERSALS:
        for knobs in (fast if trav == z.ZRT_TRAVERSAL_FAST else other):
            for k, v in knobs.items():
                monkeypatch.setenv(k, v) if v is not None else monkeypatch.delenv(k, raising=False)
            for depth in (0, 1, 2, 5, 20):
                for prng in PRNGS:
                    for flags in (0, z.ZRT_FLAG_GUARD):
                        p = z.RenderParams(24, 24, 4, depth, prng=prng, traversal=trav, flags=flags)
                        where = f"scene {which} traversal {trav} depth {depth} prng {prng} flags {flags} {knobs}"
                        monkeypatch.delenv("ZRT_STACK_LDS_ROWS16", raising=False)
                        plain = z.debug_launch_plan(view, p)
                        _check_plan(plain, depth, where)
                        monkeypatch.setenv("ZRT_STACK_LDS_ROWS16", "2")
                        capped = z.debug_launch_plan(view, p)
                        _check_plan(capped, depth, where + " rows16=2")
                        # the cap takes the FAST stack's rows out of LDS and never its 16-bit width
                        assert capped["kmode"] == plain["kmode"] and capped["stk16"] >= plain["stk16"], where
                        if plain["mode"] == 3:
                            assert capped["stack_rows"] == min(2, plain["stack_rows"]), where
                        else:
                            assert capped["stack_rows"] == plain["stack_rows"], where
                        if depth == 0:  # nothing shades: ZRT_WF=1 / ZRT_POOL=1 / the guard keep the lockstep loop
                            assert plain["sampling_loop"] in (0, 1, 2, 3, 6), where
                        n += 2
    assert n == (len(fast) + 2 * len(other)) * 5 * 2 * 2 * 2


def test_launch_plan_material_table_fallback(monkeypatch):
    """A material table past the lockstep loop's LDS share (the many-materials grid):
    FAST falls back to the wavefront loop, which reads the table from global memory -
    but not at max_depth 0, where the wavefront loop would trace and its first
    scatter write attenuation row 1 of a one-row buffer.  There the
    lockstep loop stays, without the table; the list scene falls back to the
    wave-unit loop at every depth."""
    import many_materials as M
    s = M.many_materials_scene()
    for k in LOOP_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for depth, kmode in ((0, 3), (1, 4), (2, 4), (6, 4)):
        for prng in PRNGS:
            d = z.debug_launch_plan(C.pointer(s), z.RenderParams(16, 16, 4, depth, prng=prng))
            assert (d["kmode"], d["mats_in_lds"]) == (kmode, 0), (depth, d)
            assert d["att_rows_per_path"] >= max(1, depth - 1 - d["att_rows"])
            d = z.debug_launch_plan(C.pointer(s), z.RenderParams(16, 16, 4, depth, prng=prng,
                                                                 bounded_volume_hierarchy=False))
            assert (d["mode"], d["kmode"]) == (0, 0), (depth, d)
    # a grid whose table fits keeps the lockstep loop with the table in LDS
    d = z.debug_launch_plan(C.pointer(M.many_materials_scene(M.N_SIDE_LOCKSTEP)), z.RenderParams(16, 16, 4, 6))
    assert (d["kmode"], d["mats_in_lds"]) == (3, 1), d


@pytest.mark.parametrize("index", [2, 3, 4])
def test_launch_plan_stack_row_hooks(scenes, index, monkeypatch):
    """ZRT_STACK_LDS_ROWS=<n> caps the FAST stack's LDS rows and forces the 32-bit
    stack; ZRT_STACK_LDS_ROWS16=<n> caps them the same way and keeps the 16-bit stack
    these trees (< 65 536 nodes) get, in the lockstep, wavefront and path-pool loops
    (full and compressed nodes); BINARY / REFERENCE keep their whole stack in LDS."""
    s = scenes(index)
    for env in ({"ZRT_WF": "0", "ZRT_POOL": "0"}, {"ZRT_WF": "1", "ZRT_POOL": "0"}, {"ZRT_WF": "0", "ZRT_POOL": "1"},
                {"ZRT_WF": "0", "ZRT_POOL": "1", "ZRT_QNODES": "1"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for rows in (1, 2, 4):
            p = z.RenderParams(24, 16, 4, 8)
            monkeypatch.setenv("ZRT_STACK_LDS_ROWS16", str(rows))
            d = z.debug_launch_plan(s, p)
            assert (d["stk16"], d["stack_rows"]) == (1, rows), (env, rows, d)
            assert d["qnodes"] == (1 if "ZRT_QNODES" in env else 0)
            assert d["ovf_bytes_per_lane"] == 2 * (d["stack_depth"] - rows)
            for trav in (z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE):
                b = z.debug_launch_plan(s, z.RenderParams(24, 16, 4, 8, traversal=trav))
                assert b["stack_rows"] == b["stack_depth"] and b["ovf_bytes_per_lane"] == 0
            monkeypatch.delenv("ZRT_STACK_LDS_ROWS16")
            monkeypatch.setenv("ZRT_STACK_LDS_ROWS", str(rows))
            d = z.debug_launch_plan(s, p)
            assert (d["stk16"], d["stack_rows"]) == (0, rows), (env, rows, d)
            assert d["ovf_bytes_per_lane"] == 4 * (d["stack_depth"] - rows)
            monkeypatch.delenv("ZRT_STACK_LDS_ROWS")
        monkeypatch.delenv("ZRT_QNODES", raising=False)


@pytest.mark.parametrize("index", [0, 2, 3, 4])
def test_compressed_nodes_encode_the_full_tree(scenes, index):
    """accel_build.hpp quantize_wide (DESIGN.md §3 "Compressed nodes"), on CPU: in
    every octant copy every plane decodes exactly, every slot's quantized box
    contains the full node's box, inner refs are the full node's, and every leaf
    record holds the reference leaf's box and primitive refs bit for bit - what
    wide_iter_q relies on to take wide_iter's decisions."""
    s = scenes(index)
    n = z.debug_qnodes(s)
    assert n >= 8 * 4 * 100  # 8 octant copies x 4 slots x the tree's nodes


# ---- validate_scene: every refusal, before the device check ----------------------------------

def _valid_scene():
    """A small valid scene with every kind in it: a sphere and a triangle; Lambertian
    with an image texture, metal with a colour, a dielectric (its texture index is the
    0xffffffff nobody reads).  Returns (scene, keep-alive)."""
    px = np.linspace(0.0, 1.0, 2 * 3 * 3, dtype=np.float32)
    imgs = (_ffi.Image * 1)(_ffi.Image(3, 2, px.ctypes.data_as(C.POINTER(C.c_float))))
    texs = (_ffi.Texture * 2)(_ffi.Texture(_ffi.ZRT_TEX_IMAGE, 0, _ffi.Vec3(0, 0, 0), -0.3, 0.35),
                              _ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0.5, 0.5, 0.5), 0.0, 0.0))
    mats = (_ffi.Material * 3)(_ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 0, 0.0),
                               _ffi.Material(_ffi.ZRT_MAT_METAL, 1, 0.0),
                               _ffi.Material(_ffi.ZRT_MAT_DIELECTRIC, 0xFFFFFFFF, 1.5))
    prims = (_ffi.Prim * 3)()
    prims[0].kind, prims[0].material = _ffi.ZRT_PRIM_SPHERE, 0
    prims[0].center, prims[0].radius = _ffi.Vec3(0, 0, 3), 1.0
    prims[1].kind, prims[1].material = _ffi.ZRT_PRIM_TRIANGLE, 1
    prims[1].a, prims[1].b, prims[1].c = _ffi.Vec3(-1, -1, 2), _ffi.Vec3(0, 1, 2.5), _ffi.Vec3(1, -1, 2)
    prims[2].kind, prims[2].material = _ffi.ZRT_PRIM_SPHERE, 2
    prims[2].center, prims[2].radius = _ffi.Vec3(1, 0, 2), 0.5
    s = _ffi.Scene(prims, 3, 3, mats, texs, 2, 1, imgs)
    return s, (prims, mats, texs, imgs, px)


def _set(path, value):
    def mutate(s, keep):
        obj = s
        *head, last = path
        for step in head:
            obj = getattr(obj, step[0])[step[1]] if isinstance(step, tuple) else getattr(obj, step)
        setattr(obj, last, value)
    return mutate


REFUSALS = [
    ("prim-kind", _set([("prims", 1), "kind"], 2), "unknown primitive kind"),
    ("prim-material", _set([("prims", 2), "material"], 3), "material index out of range"),
    ("material-kind", _set([("materials", 1), "kind"], 3), "unknown material kind"),
    ("material-texture", _set([("materials", 0), "texture"], 2), "texture index out of range"),
    ("metal-texture-unset", _set([("materials", 1), "texture"], 0xFFFFFFFF), "texture index out of range"),
    ("texture-kind", _set([("textures", 1), "kind"], 2), "unknown texture kind"),
    ("texture-image", _set([("textures", 0), "image"], 1), "image index out of range"),
    ("image-null-pixels", _set([("images", 0), "pixels"], C.POINTER(C.c_float)()), "empty image"),
    ("image-width-0", _set([("images", 0), "width"], 0), "empty image"),
    ("image-height-0", _set([("images", 0), "height"], 0), "empty image"),
    ("null-prims", _set(["prims"], C.POINTER(_ffi.Prim)()), "prims is null"),
    ("null-materials", _set(["materials"], C.POINTER(_ffi.Material)()), "materials is null"),
    ("null-textures", _set(["textures"], C.POINTER(_ffi.Texture)()), "textures is null"),
    ("null-images", _set(["images"], C.POINTER(_ffi.Image)()), "images is null"),
]


def _scene_calls(s):
    """The three entry points of the issue, each on scene s: context creation, the
    one-shot render and the device-free launch plan."""
    view = C.pointer(s)
    cam = z.camera_init((0, 0, -1), (0, 0, 3), (0, 1, 0), 45.0, 1.0)
    p = z.RenderParams(8, 8, 1, 4)
    return {"zrt_ctx_create": lambda: z.RenderContext(view, p),
            "zrt_render": lambda: z.render(view, cam, p),
            "zrt_debug_launch_plan": lambda: z.debug_launch_plan(view, p)}


@pytest.mark.parametrize("name,mutate,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_validate_scene_refusals(name, mutate, message):
    """planner.cpp validate_scene: each refusal, reached by changing one field of a valid
    scene, comes back as ZRT_E_INVALID with its own message from zrt_ctx_create,
    zrt_render and zrt_debug_launch_plan - before the device check, so with no GPU too."""
    s, keep = _valid_scene()
    mutate(s, keep)
    for entry, call in _scene_calls(s).items():
        with pytest.raises(z.ZrtError) as e:
            call()
        assert e.value.code == _ffi.ZRT_E_INVALID, (entry, str(e.value))
        assert message in str(e.value), (entry, str(e.value))


def test_validate_scene_accepts_the_unmutated_scene():
    """The scene the refusals start from is valid - its dielectric's texture index is
    0xffffffff, which validate_scene and the flattening skip.  Past validation a launch
    plan is made and the LDS plans of the flattened scene are checked, and without a
    GPU the entry points that need one report ZRT_E_NODEVICE, not ZRT_E_INVALID."""
    s, keep = _valid_scene()
    assert s.materials[2].kind == _ffi.ZRT_MAT_DIELECTRIC and s.materials[2].texture == 0xFFFFFFFF
    calls = _scene_calls(s)
    d = calls["zrt_debug_launch_plan"]()
    assert d["mode"] == 0 and d["sampling_loop"] in (0, 6)  # (3 primitives: the surface list)
    assert z.debug_lds_plans(C.pointer(s)) > 0
    import torch
    if not torch.cuda.is_available():
        for entry in ("zrt_ctx_create", "zrt_render"):
            with pytest.raises(z.ZrtError) as e:
                calls[entry]()
            assert e.value.code == _ffi.ZRT_E_NODEVICE, entry
    # the same scene as the oracle reads it: a frame without NaN
    cam = z.camera_init((0, 0, -1), (0, 0, 3), (0, 1, 0), 45.0, 1.0)
    img, st = O.render(C.pointer(s), cam, z.RenderParams(8, 8, 2, 4))
    assert np.isfinite(img).all() and st["reflections"] > 0

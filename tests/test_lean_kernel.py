"""The host's choice of the lean lockstep kernel (no device).

render.hip compiles the timed lockstep FAST kernel a second time without image
textures, dielectrics, the ray-origin check and the
scanline rows (render.hip struct Lean).  zrt_ctx_render_tiles launches it only where the
scene, the params and the camera allow it (plan_launch's `lean`, lean_launch);
zrt_debug_lean_kernel reports that decision through the same functions.

Invariant: the lean kernel is never chosen for a scene with a dielectric, an
image texture or a triangle past the fast 1/det bound, with scanline rows, at
depth 0, for the STATS flavour, from a camera outside the origin bound, for
another loop than the lockstep FAST one, or under ZRT_LEAN=0.  The scene facts
are recomputed here from the zrt_scene itself, not read back from the library.
"""
import ctypes as C

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi

import lean_scenes as LS

PRNGS = (z.ZRT_PRNG_XOROSHIRO128, z.ZRT_PRNG_XOSHIRO256)
DEFAULT_ON = True  # planner.cpp lean_wanted: an eligible launch is lean with ZRT_LEAN unset
REFERENCE_SCENES = [0, 1, 2, 3, 4, 6]
# the mesh scenes of solid Lambertian and metal materials only (scenes.zig): lean by default
SOLID_MESH_SCENES = [0, 2, 3]


def scene_of(scenes, which):
    """(keep-alive, zrt_scene pointer, camera, camera inside the origin bound)."""
    if which in LS.NAMES:
        keep, view, cam = LS.get(which)
        return keep, view, cam, which != "d"
    s = scenes(which)
    return s, s.view, s.camera, True  # (the reference scenes' cameras lie inside their bounds)


def scene_facts(view):
    """has_dielectric, has_image_texture, every triangle's |n| components < 2^124 -
    from the zrt_scene's own arrays."""
    s = view.contents
    diel = image = False
    for i in range(s.n_materials):
        m = s.materials[i]
        if m.kind == _ffi.ZRT_MAT_DIELECTRIC:
            diel = True
        elif s.textures[m.texture].kind == _ffi.ZRT_TEX_IMAGE:
            image = True
    words = C.sizeof(_ffi.Prim) // 4
    raw = np.frombuffer(C.string_at(s.prims, s.n_prims * C.sizeof(_ffi.Prim)), dtype=np.uint32).reshape(-1, words)
    tri = raw[raw[:, 0] == _ffi.ZRT_PRIM_TRIANGLE]
    f = tri[:, 6:15].view(np.float32).astype(np.float64)  # a, b, c
    n = np.cross(f[:, 3:6] - f[:, 0:3], f[:, 6:9] - f[:, 0:3])
    # (the margin of the f32 cross product against this f64 one is far inside 2^124 / 2)
    fast = bool((np.abs(n) < 2.0 ** 123).all()) if len(n) else True
    return diel, image, fast


@pytest.mark.parametrize("which", REFERENCE_SCENES + list(LS.NAMES))
def test_lean_choice_invariant(scenes, which, monkeypatch):
    """Scenes 0-4 and 6 and the four synthetic scenes x depth 0, 1, 20 x both PRNGs x
    ZRT_FLAG_SCANLINES x ZRT_FLAG_GUARD x ZRT_FLAG_STATS x ZRT_LEAN unset, 0, 1."""
    _, view, cam, inside = scene_of(scenes, which)
    diel, image, fast = scene_facts(view)
    n_lean = 0
    # (scene 6, 1.6 M triangles, flattens in seconds a call: its image textures are
    # tried once, at the benchmark's depth with the knob asking for the lean kernel)
    big = which == 6
    for depth in ((20,) if big else (0, 1, 20)):
        for prng in (PRNGS[:1] if big else PRNGS):
            for flags in ((0,) if big else (0, z.ZRT_FLAG_SCANLINES, z.ZRT_FLAG_GUARD,
                                            z.ZRT_FLAG_SCANLINES | z.ZRT_FLAG_GUARD, z.ZRT_FLAG_STATS)):
                p = z.RenderParams(24, 24, 4, depth, prng=prng, flags=flags)
                # (ZRT_LEAN changes nothing zrt_debug_launch_plan reports)
                plan = {"kmode": 4, "mats_in_lds": 0} if big else z.debug_launch_plan(view, p)
                eligible = (plan["kmode"] == 3 and plan["mats_in_lds"] == 1 and depth >= 1 and not diel
                            and not image and fast and inside
                            and not flags & (z.ZRT_FLAG_SCANLINES | z.ZRT_FLAG_STATS))
                for knob in (("1",) if big else (None, "0", "1")):
                    if knob is None:
                        monkeypatch.delenv("ZRT_LEAN", raising=False)
                    else:
                        monkeypatch.setenv("ZRT_LEAN", knob)
                    where = f"scene {which} depth {depth} prng {prng} flags {flags} ZRT_LEAN={knob}"
                    lean = z.debug_lean_kernel(view, cam, p)
                    if lean:
                        assert eligible and knob != "0", where
                        n_lean += 1
                    # the knob decides among eligible launches only, and decides them
                    want = eligible and (DEFAULT_ON if knob is None else knob == "1")
                    assert lean == want, where
    if which in SOLID_MESH_SCENES + ["a"]:
        assert n_lean > 0, "an eligible scene never takes the lean kernel"
    if which in (1, 4, 6, "b", "c", "d"):
        # (1: a list of spheres, with glass; 4, 6: image textures; b-d: ineligible by construction)
        assert n_lean == 0, which
        assert which == 1 or diel or image or not inside, which


def test_synthetic_scene_facts():
    """The four synthetic scenes are what they are meant to be: only b has a
    dielectric, only c an image texture, all have a BVH, and only d's camera lies
    outside the origin bound (the lean choice differs between a and d by the camera alone)."""
    p = z.RenderParams(24, 24, 4, 6)
    for name in LS.NAMES:
        _, view, cam, _ = scene_of(None, name)
        diel, image, fast = scene_facts(view)
        assert (diel, image, fast) == (name == "b", name == "c", True), name
        assert view.contents.n_prims > 10 and z.debug_launch_plan(view, p)["kmode"] == 3, name
    _, va, ca, _ = scene_of(None, "a")
    _, vd, cd, _ = scene_of(None, "d")
    os_env_free = z.RenderParams(24, 24, 4, 6)
    assert z.debug_lean_kernel(va, ca, os_env_free) == DEFAULT_ON
    assert not z.debug_lean_kernel(vd, cd, os_env_free)
    assert not z.debug_lean_kernel(va, cd, os_env_free)  # a's scene from d's camera


def test_solid_mesh_scenes_are_lean_by_default(scenes, monkeypatch):
    """Scenes 0, 2 and 3 (and synthetic a) at the benchmark's settings take the lean
    kernel when it is the default, always with ZRT_LEAN=1 and never with ZRT_LEAN=0."""
    for which in SOLID_MESH_SCENES + ["a"]:
        _, view, cam, _ = scene_of(scenes, which)
        p = z.RenderParams(64, 64, 8, 20)
        monkeypatch.delenv("ZRT_LEAN", raising=False)
        assert z.debug_lean_kernel(view, cam, p) == DEFAULT_ON, which
        monkeypatch.setenv("ZRT_LEAN", "1")
        assert z.debug_lean_kernel(view, cam, p), which
        monkeypatch.setenv("ZRT_LEAN", "0")
        assert not z.debug_lean_kernel(view, cam, p), which


@pytest.mark.parametrize("which", list(LS.NAMES))
def test_synthetic_scenes_plans(which):
    """zrt_debug_lds_plans and zrt_debug_buffer_plans hold for the synthetic scenes too
    (tests/test_host.py runs them over the reference scenes, unchanged)."""
    _, view, _, _ = scene_of(None, which)
    assert z.debug_lds_plans(view) > 0
    assert z.debug_buffer_plans(view) > 0

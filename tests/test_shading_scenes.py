"""The scenes of tests/shading_scenes.py reach the branches they are named for.

CPU only.  tests/test_gpu_shading_edges.py renders these scenes in every sampling
loop and compares with the oracle; a frame can only differ in a branch that some
path takes.  Here the 24 x 24 pixel-centre primary rays of each scene are
classified with the oracle's closest hit and hit records plus f32 restatements of
HitRecord's front test, the dielectric's ratio * sin_theta, the triangle's
barycentric (u, v) and the arms of the texture wrap (shading_scenes.classify), and
every class needs at least MIN_RAYS of the 576 rays - as
test_hazard_rays_reach_the_band pins the order-hazard construction.

Also, with no device: none of the scenes is eligible for the lean kernel, every
LDS / buffer plan and the compressed nodes pass their host-side checks, and each
loop of test_gpu_loop_edges.LOOPS is the one the launch plan takes.
"""
import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O

import shading_scenes as S
import test_gpu_loop_edges as E

MIN_RAYS = 16

WRAP_ARMS = ["uu_first < 0", "uu_first > 1", "vv_first > 1", "vv_first < 0 kept", "quirk past 1"]
CLASSES = {
    # dielectric first hits from the back, past the critical angle and under it
    "glass-inside": ["dielectric back TIR", "dielectric back Schlick"],
    # total internal reflection at a front hit (ior < 1), glass and textured metal on the mesh,
    # and the hollow shell's inner sphere met from the back by the rays refracted into the glass
    "bubbles": ["dielectric front TIR", "dielectric front Schlick", "dielectric triangle", "image metal triangle",
                "image lambertian triangle", "shell inside back"],
    "wraps": WRAP_ARMS + ["image 0", "image 1", "image 2", "image 3", "image metal triangle", "image metal sphere",
                          "image lambertian triangle", "image lambertian sphere"],
    "poles": ["theta < 2^-10", "seam, u near 0", "seam, u near 1", "uu_first < 0", "vv_first < 0 kept", "quirk"],
}

_COUNTS = {}


def counts(name):
    if name not in _COUNTS:
        _COUNTS[name] = S.classify(O, name)
    return _COUNTS[name]


@pytest.mark.parametrize("name", S.NAMES)
def test_primary_rays_reach_their_classes(name):
    n = counts(name)
    print(name, sorted(n.items()))
    assert n["rays"] == 576
    for cls in CLASSES[name]:
        assert n.get(cls, 0) >= MIN_RAYS, (cls, n.get(cls, 0))
    if name == "glass-inside":  # every primary ray starts inside the glass
        assert n["dielectric sphere"] == 576 == n["dielectric back TIR"] + n["dielectric back Schlick"]
    if name == "bubbles":  # no dielectric is seen from inside; the shell's inner sphere only from the back
        assert "dielectric back TIR" not in n and "dielectric back Schlick" not in n
        assert "shell inside front" not in n
    if name == "poles":
        assert n["pole"] == 576
        # |outward.y| > 1 (acos gives NaN) is not reached by this geometry; if a change of
        # the geometry reaches it, it has to be reached with room like every other class
        assert n.get("theta NaN", 0) == 0 or n["theta NaN"] >= MIN_RAYS


def test_wraps_images_and_stores():
    """The four images: two with arbitrary f32 values and two exact k / 255, one of
    each kind first in its device store and one behind it; 1 texel wide, 1 texel high
    and 1 x 1 among them; every texel of an image differs from the others."""
    imgs = S.images()
    assert [(a.shape[1], a.shape[0]) for a in imgs] == [(1, 1), (5, 3), (1, 7), (8, 2)]
    exact = [bool((np.round(a * np.float32(255.0)).astype(np.float32) / np.float32(255.0) == a).all()) for a in imgs]
    assert exact == [False, False, True, True]
    for a in imgs:
        texels = a.reshape(-1, 3)
        assert len({t.tobytes() for t in texels}) == len(texels)
    s, _, _ = S.get("wraps")
    used = {(s.textures[s.materials[s.prims[i].material].texture].image,
             s.textures[s.materials[s.prims[i].material].texture].u_offset)
            for i in range(s.n_prims) if s.textures[s.materials[s.prims[i].material].texture].kind == 1}
    assert {i for i, _ in used} == {0, 1, 2, 3}
    assert {u for _, u in used} == {np.float32(-0.3), np.float32(1.25), np.float32(0.0)}


@pytest.mark.parametrize("name", S.NAMES)
def test_host_side_plans(name, monkeypatch):
    """No device: the lean kernel is not chosen (every scene has a dielectric or an
    image texture), the LDS plans, the shared-buffer plans and the compressed nodes
    pass, and each loop of test_gpu_loop_edges.LOOPS is planned as its entry says -
    the list loops with bounded_volume_hierarchy off, the material table in LDS for
    the loops that read it there only."""
    s, view, cam = S.get(name)
    assert 11 <= s.n_prims < 40
    monkeypatch.delenv("ZRT_LEAN", raising=False)
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES"):
        monkeypatch.delenv(k, raising=False)
    for prng in E.PRNGS.values():
        assert not z.debug_lean_kernel(view, cam, z.RenderParams(24, 24, 4, 12, prng=prng, sample_chunk=3))
    assert z.debug_lds_plans(view) > 0
    assert z.debug_buffer_plans(view) > 0
    assert z.debug_qnodes(view) > 0
    for loop, (_, _, _, want) in E.LOOPS.items():
        for depth in (2, 12):
            for prng in E.PRNGS.values():
                p = z.RenderParams(24, 24, 4, depth, prng=prng, sample_chunk=3,
                                   bounded_volume_hierarchy=loop not in E.LIST_LOOPS)
                p = E.set_edge_loop(monkeypatch, loop, p)
                d = z.debug_launch_plan(view, p)
                assert d["sampling_loop"] == want, (loop, depth, d)
                mode = 0 if loop in E.LIST_LOOPS else {E.FAST: 3, E.BINARY: 1, E.REFERENCE: 2}[p.traversal]
                assert d["mode"] == mode, (loop, depth, d)
                if d["kmode"] in (3, 6):
                    assert d["mats_in_lds"] == 1, (loop, d)
                assert d["qnodes"] == (1 if loop == "pool-qnodes" else 0)

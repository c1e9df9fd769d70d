"""Material.scatter and the texture lookup at their edges, in every sampling loop.

render.hip writes the scatter out three times (shade_step in its general and
its lean form, shade_hit_a with the materials' shared operations issued once per wave) and the texture lookup once (image_texel_code); the
reference scenes reach few of their branches.  The scenes of
tests/shading_scenes.py reach the others - tests/test_shading_scenes.py proves it
on the CPU, ray by ray:

* total internal reflection (ratio * sin_theta > 1, material.zig:116) at back
  hits (a camera inside glass, a hollow shell's inner sphere) and at front hits
  (a sphere with ior < 1);
* dielectric first hits from the back (front_face false, ratio = ior), ior = 1;
* glass and image-textured metal on triangles (the barycentric (u, v));
* every arm of the texture wrap (texture.zig:52-74) with negative offsets and
  offsets past 1, the V wrap that tests uu_first (:66), negative and over-range
  texel coordinates; images 1 texel wide and high; a second image in each device
  texel store (img_off != 0);
* a sphere's pole (theta = acos(-outward.y) at and near 0) and the meridian where
  atan2 jumps (sphere.zig:47-50).

Every case compares with the oracle bit for bit through test_gpu_loop_edges's
check_frame: the image (NaN included), the Progress counters, the scanline rows,
the STATS flavour's bits, and the sampling loop that ran.  Before a comparison the
oracle's own counters show that paths scatter and reach the depth limit, so that
no case passes on a frame of misses.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import pytest

import zraytrace_amd as z

import shading_scenes as S
import test_gpu_loop_edges as E

pytestmark = pytest.mark.gpu

# (scene, max_depth): every scene at depth 12; "glass-inside" also at 2, where the first
# scatter - reflect past the critical angle or by Schlick's draw, else refract - decides the frame
FRAMES = [(name, 12) for name in S.NAMES] + [("glass-inside", 2)]


def not_vacuous(scenes, name, p):
    """From the oracle's own counters: paths scatter (more reflections than samples)
    and, with max_depth 2, some end at the depth limit."""
    rs = E.oracle_frame(scenes, name, p)[1]
    assert rs["samples_processed"] == p.width * p.height * p.samples_per_pixel
    assert rs["reflections"] > rs["samples_processed"], rs
    assert E.depth_hits(scenes, name, p, 2) > 0


@pytest.mark.parametrize("prng", list(E.PRNGS))
@pytest.mark.parametrize("loop", E.BVH_LOOPS + E.LIST_LOOPS)
@pytest.mark.parametrize("name,max_depth", FRAMES, ids=[f"{n}-d{d}" for n, d in FRAMES])
def test_shading_edges_every_loop(scenes, name, max_depth, loop, prng, monkeypatch):
    """24 x 24, 4 spp in chunks of 3: the BVH loops on the scene's tree, the list loops
    on the same scene with bounded_volume_hierarchy off (shade_hit_a), both generators."""
    p = E.frame_params(max_depth, E.PRNGS[prng])
    p = dataclasses.replace(p, bounded_volume_hierarchy=loop not in E.LIST_LOOPS)
    p = E.set_edge_loop(monkeypatch, loop, p)
    not_vacuous(scenes, name, p)
    gs, rs = E.check_frame(scenes, name, p)
    assert rs["used_bvh"] == (0 if loop in E.LIST_LOOPS else 1)
    _, view, _ = E.scene_of(scenes, name)
    assert gs["sampling_loop"] == z.debug_launch_plan(view, p)["sampling_loop"] == E.LOOPS[loop][3]
    if name in ("wraps", "poles"):
        assert gs["texel_bytes"] == 12  # (f32 images in the scene: both texel stores are in use)
    if name == "glass-inside":
        assert gs["texel_bytes"] == 0


@pytest.mark.parametrize("name", S.NAMES)
def test_shading_edges_behind_the_probe(scenes, name, monkeypatch):
    """16 x 16 at 128 spp: the scheduling probe's own lockstep launch shades these
    scenes first, then the default FAST loop renders them in its order."""
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES"):
        monkeypatch.delenv(k, raising=False)
    p = E.frame_params(12, w=16, h=16, spp=128, chunk=0)
    not_vacuous(scenes, name, p)
    gs, rs = E.check_frame(scenes, name, p, scanlines=False)
    _, view, _ = E.scene_of(scenes, name)
    assert gs["schedule_ms"] > 0 and gs["sampling_loop"] == z.debug_launch_plan(view, p)["sampling_loop"]


@pytest.mark.parametrize("loop", E.BVH_LOOPS + E.LIST_LOOPS)
def test_texel_codes_through_global_attenuation_rows(scenes, loop, monkeypatch):
    """ZRT_ATT_LDS_ROWS=0 on "wraps": every attenuation code a path stacks - texel
    indices of both stores among them - goes through the global rows."""
    monkeypatch.setenv("ZRT_ATT_LDS_ROWS", "0")
    p = E.frame_params(12)
    p = dataclasses.replace(p, bounded_volume_hierarchy=loop not in E.LIST_LOOPS)
    p = E.set_edge_loop(monkeypatch, loop, p)
    _, view, _ = E.scene_of(scenes, "wraps")
    plan = z.debug_launch_plan(view, p)
    assert plan["att_rows"] == 0 and plan["att_rows_per_path"] >= 11
    not_vacuous(scenes, "wraps", p)
    gs, rs = E.check_frame(scenes, "wraps", p)
    assert gs["sampling_loop"] == E.LOOPS[loop][3] and gs["texel_bytes"] == 12
    assert E.depth_hits(scenes, "wraps", p, 3) > 0  # (paths scatter three times: rows are written and read back)

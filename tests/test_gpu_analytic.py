"""GPU tests: every kernel that produces radiance against the closed forms of
tests/analytic_ref.py and tests/analytic_frames.py - never against the oracle (test_gpu_radiance.py and the others do
that): these assertions would hold or fail without oracle.c existing.

The rule, the cases and the sample counts are those of tests/test_analytic_ref.py:
|mean - expected| <= 5 sqrt(var / N) + floor per channel, var in closed form, 4096 streams of
256 samples along a case's ray (N = 2^20), means averaged in float64 on the host.

1. zrt_ctx_radiance: every case, list and BVH-padded, FAST / BINARY / REFERENCE, both PRNGs,
   the info counters held to the exact and the expected counts;
2. the frame loops through z.render on the degenerate camera, each loop by name;
3. zrt_ctx_camera through the five lenses on the floor, the pinhole's sky rows by quadrature;
4. the same pinhole frames through z.render, with and without sky_kernel;
5. zrt_render_ao on the floor under the sphere against 1 - r^2 cos(beta) / d^2;
6. the far end of the key's sample and ray fields.

Run on an MI355X: ``pytest -m gpu``.
"""
import functools

import numpy as np
import pytest

import analytic_frames as AF
import analytic_ref as A
import radiance_ref as R
import test_analytic_ref as T
import test_gpu_loop_edges as E
import zraytrace_amd as z

pytestmark = pytest.mark.gpu
F = np.float32
FAST, BINARY, REFERENCE = z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_BINARY, z.ZRT_TRAVERSAL_REFERENCE
TRAVERSALS = {"fast": FAST, "binary": BINARY, "reference": REFERENCE}
PRNGS = T.PRNGS
N_RAYS, SPP, CHUNK = 4096, 256, 32
N = N_RAYS * SPP


def rparams(c, bvh, prng, trav=FAST, side=1, spp=1):
    return z.RenderParams(side, side, spp, c.depth, bounded_volume_hierarchy=bvh, prng=prng, traversal=trav,
                          sample_chunk=CHUNK)


def check_mean(c, mean, n, what, spp=SPP):
    ok, zs = A.accept(mean, c.mean(), c.var, n, T.margin(c, spp))
    print(f"{what}: N {n} dev {np.abs(mean - c.mean()).max():.3e} z {zs.max():.2f}")
    assert ok.all(), f"{what}: mean {mean} against {c.mean()}, z {zs}"


@functools.lru_cache(maxsize=None)
def device_rays(name):
    import torch
    o, d = A.cases()[name].ray()
    rays = np.tile(np.concatenate([o, d]).astype(F), (N_RAYS, 1))
    return torch.from_numpy(np.ascontiguousarray(rays)).cuda()


def query(ctx, p, name, first_sample=0, first_ray=0):
    """One zrt_ctx_radiance call over 4096 copies of the case's ray, as rays first_ray ..
    first_ray + 4095: (mean of the per-ray means in float64, info)."""
    import torch
    rays = device_rays(name)
    s = torch.zeros((N_RAYS, 4), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((N_RAYS, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.radiance(p, z.radiance_settings(SPP, first_sample, first_ray), rays.data_ptr(), N_RAYS, s.data_ptr(), rgb.data_ptr())
    ctx.sync()
    torch.cuda.synchronize()
    return rgb.cpu().numpy().astype(np.float64).mean(0), ctx.radiance_info()


# ---- 1. zrt_ctx_radiance ------------------------------------------------------------------

@pytest.mark.parametrize("prng", list(PRNGS))
@pytest.mark.parametrize("name,bvh", T.VARIANTS, ids=T.IDS)
def test_radiance_meets_the_closed_form(name, bvh, prng):
    c = A.cases()[name]
    _, view = c.scene(bvh)
    ctx = z.RenderContext(view, rparams(c, bvh, PRNGS[prng]))
    try:
        # (the surface list is walked in the reference's order whatever the traversal)
        for tn, trav in TRAVERSALS.items() if bvh else (("fast", FAST), ("reference", REFERENCE)):
            what = f"{name} {'bvh' if bvh else 'list'} {prng} {tn}"
            mean, info = query(ctx, rparams(c, bvh, PRNGS[prng], trav), name)
            assert info["samples"] == N
            check_mean(c, mean, N, what)
            if c.counters is not None:
                T.check_counters(c, info, N, what)
    finally:
        ctx.close()


# ---- 2. the frame loops -------------------------------------------------------------------

# loop -> (loop of test_gpu_loop_edges, ZRT_LEAN, the plan's kmode and qnodes)
FRAME_LOOPS = {"lockstep-full": ("lockstep", "0", 3, 0), "lockstep-lean": ("lockstep", "1", 3, 0),
               "wavefront": ("wavefront", None, 4, 0), "pool": ("pool", None, 5, 0), "pool-qnodes": ("pool-qnodes", None, 8, 1),
               "binary": ("binary", None, 1, 0), "reference": ("reference", None, 2, 0),
               "list-items": ("list-items", None, 6, 0), "list-wave": ("list-wave", None, 0, 0)}
# a BVH-padded case of (a), (c) and (e); of these only (e)'s scene fits the lean kernel
FRAME_CASES = {"lambert-sphere-generic-d2": False, "glass-0.6667-generic-d50": False, "occluded-floor-tilted": True}


@pytest.mark.parametrize("loop", list(FRAME_LOOPS))
@pytest.mark.parametrize("name", list(FRAME_CASES))
def test_frame_loops_meet_the_closed_form(name, loop, monkeypatch):
    """A 64 x 64 frame of 256 samples on the degenerate camera: 4096 streams along the case's
    ray, through the loop the test names - the stats and the plan must say so."""
    c = A.cases()[name]
    edge, lean_knob, kmode, qnodes = FRAME_LOOPS[loop]
    bvh = edge not in E.LIST_LOOPS
    _, view = c.scene(bvh)
    cam = R.ray_camera(c.o, c.tgt)
    p = E.set_edge_loop(monkeypatch, edge, rparams(c, bvh, PRNGS["xoroshiro"], side=64, spp=SPP))
    monkeypatch.delenv("ZRT_LEAN", raising=False)
    if lean_knob is not None:
        monkeypatch.setenv("ZRT_LEAN", lean_knob)
    plan = z.debug_launch_plan(view, p)
    lean = z.debug_lean_kernel(view, cam, p)
    assert (plan["kmode"], plan["qnodes"]) == (kmode, qnodes)
    assert lean == (loop == "lockstep-lean" and FRAME_CASES[name]), "the lean kernel's eligibility changed"
    img, st = z.render(view, cam, p)
    assert st["sampling_loop"] == plan["sampling_loop"] == E.LOOPS[edge][3] and st["used_bvh"] == int(bvh)
    assert st["samples_processed"] == N
    what = f"{name} {loop}"
    check_mean(c, img.astype(np.float64).reshape(-1, 3).mean(0), N, what)
    if c.counters is not None:
        T.check_counters(c, {k: st[v] for k, v in T._STATS.items()}, N, what)


# ---- 3. zrt_ctx_camera through the five lenses ----------------------------------------------

LENSES = {"pinhole": z.ZRT_LENS_PINHOLE, "thin": z.ZRT_LENS_THIN, "ortho": z.ZRT_LENS_ORTHO,
          "equirect": z.ZRT_LENS_EQUIRECT, "fisheye": z.ZRT_LENS_FISHEYE}
# (pose, the fewest floor pixels the frame must hold): the horizon frame, and one that looks down
POSES = {"horizon": AF.FRAME_POSE, "down": AF.DOWN_POSE}
# (an orthographic lens that looks up at the horizon sees no floor: it only looks down)
FLOOR_PIXELS = {("pinhole", "horizon"): 96, ("thin", "horizon"): 80, ("equirect", "horizon"): 112, ("fisheye", "horizon"): 96,
                ("pinhole", "down"): 256, ("thin", "down"): 256, ("ortho", "down"): 256,
                ("equirect", "down"): 112, ("fisheye", "down"): 160}


@pytest.mark.parametrize("kind,pose", list(FLOOR_PIXELS), ids=[f"{k}-{p}" for k, p in FLOOR_PIXELS])
@pytest.mark.parametrize("prng", list(PRNGS))
def test_camera_queries_meet_the_floor_constant(kind, pose, prng):
    """16 x 16, 1024 samples, the floor alone: every pixel whose footprint - over the whole lens
    disc of a thin lens of aperture 0.5 - lies on the floor is rho sky(2/3), whatever the lens;
    the pinhole's sky pixels are the quadrature of the sky over the footprint."""
    lens = z.lens_init(LENSES[kind], *POSES[pose], aperture=0.5, focus_dist=4.0, fisheye_fov=120.0)
    cls = AF.classify_pixels(lens, LENSES[kind])
    assert int((cls == 1).sum()) >= FLOOR_PIXELS[kind, pose]
    _, view = AF.floor_scene()
    p = z.RenderParams(AF.FRAME_W, AF.FRAME_H, 1, 4, prng=PRNGS[prng], sample_chunk=CHUNK)
    rgb, info = z.render_lens(view, p, lens, T.FRAME_SPP)
    assert info["samples"] == 256 * T.FRAME_SPP
    bad, _ = T.check_frame(rgb.astype(np.float64), cls, lens if kind == "pinhole" else None, T.FRAME_SPP,
                           f"{kind} {pose} {prng}")
    assert not bad, bad


# ---- 4. the pinhole frames through z.render -------------------------------------------------

@pytest.mark.parametrize("prng", list(PRNGS))
@pytest.mark.parametrize("bvh", [False, True], ids=["list", "bvh-tilted"])
def test_rendered_floor_frame(bvh, prng, monkeypatch):
    """FRAME_POSE on the floor through the frame path: the list loop on the flat floor, the
    shipped BVH loop on the tilted, padded one (rho sky((2/3) n_y); its far side rises, so the
    horizon crosses row 7 alone)."""
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES", "ZRT_LEAN", "ZRT_SKY_TILES"):
        monkeypatch.delenv(k, raising=False)
    cam = z.camera_init(*AF.FRAME_POSE)
    tri = A.tilted_floor(0.05) if bvh else A.FLOOR
    cls = AF.classify_pixels(cam, z.ZRT_LENS_PINHOLE, tri=tri)
    assert (cls[:7 if bvh else 6] == 1).all() and (cls[8:] == 2).all()
    _, view = AF.floor_scene(bvh, 0.05 if bvh else 0.0)
    p = z.RenderParams(AF.FRAME_W, AF.FRAME_H, T.FRAME_SPP, 4, bounded_volume_hierarchy=bvh, prng=PRNGS[prng], sample_chunk=CHUNK)
    img, st = z.render(view, cam, p)
    assert st["used_bvh"] == int(bvh)
    bad, _ = T.check_frame(img.astype(np.float64), cls, cam, T.FRAME_SPP, f"floor frame bvh {bvh} {prng}",
                           floor_ny=A.tri_normal(*tri)[1])
    assert not bad, bad


@pytest.mark.parametrize("knob", ["1", "0"], ids=["sky-kernel", "traversal"])
def test_rendered_sky_meets_the_quadrature(knob, monkeypatch):
    """SPHERE_POSE at the BVH-padded unit sphere: the two upper tiles are all sky - as shipped
    sky_kernel renders them, under ZRT_SKY_TILES=0 the lockstep kernel does - and the lower
    tiles' sky pixels go through traversal either way: every one the quadrature."""
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES", "ZRT_LEAN"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ZRT_SKY_TILES", knob)
    cam = z.camera_init(*AF.SPHERE_POSE)
    cls = AF.sky_pixels_beside_sphere(cam, (0.0, 0.0, 0.0), 1.0)
    assert (cls[8:] == 2).all() and int((cls[:8] == 2).sum()) >= 64
    _, view = A.cases()["lambert-sphere-generic-d2"].scene(True)
    p = z.RenderParams(AF.FRAME_W, AF.FRAME_H, T.FRAME_SPP, 4, sample_chunk=CHUNK)
    n_sky = int((z.debug_tile_classes(view, cam, p)[0] == z.ZRT_TILE_SKY).sum())
    assert n_sky == (2 if knob == "1" else 0)
    img, st = z.render(view, cam, p)
    assert st["sampling_loop"] == 3
    bad, _ = T.check_frame(img.astype(np.float64), cls, cam, T.FRAME_SPP, f"sky frame, ZRT_SKY_TILES={knob}")
    assert not bad, bad


# ---- 5. ambient occlusion -----------------------------------------------------------------

AO_N = {"atomic": 1024, "wave": 64}


@pytest.mark.parametrize("reduction", list(AO_N))
@pytest.mark.parametrize("bvh", [False, True], ids=["list", "bvh-tilted"])
def test_ao_meets_the_form_factor(bvh, reduction):
    """16 x 16 floor pixels under and beside (e)'s sphere: ao(p) against 1 - (r / d)^2 cos(beta)
    at the centre ray's hit point (r^2 h / d^3 on the flat floor), variance p (1 - p) / n per
    pixel, and the pixels' mean deviation together; both reductions, every traversal."""
    c = A.cases()["occluded-floor-tilted" if bvh else "occluded-floor"]
    _, view = c.scene(bvh)
    cam = z.camera_init(*AF.AO_POSE)
    n = AO_N[reduction]
    tri, centre = c.tris[0][:3], np.array(c.spheres[0][0])
    want = AF.ao_expected(cam, 16, 16, tri, centre, A.OCC_R)
    floor = ~np.isnan(want)
    assert floor.sum() >= 200 and np.nanmin(want) < 0.7 and np.nanmax(want) > 0.99
    plan = z.debug_ao_plan(z.RenderParams(16, 16, 1, 4), z.ao_settings(n))
    assert plan["reduction"] == (z._ffi.ZRT_AO_REDUCE_ATOMIC if reduction == "atomic" else z._ffi.ZRT_AO_REDUCE_WAVE)
    for tn, trav in TRAVERSALS.items() if bvh else (("fast", FAST),):
        p = z.RenderParams(16, 16, 1, 4, bounded_volume_hierarchy=bvh, traversal=trav)
        ao, clear, feat = z.render_ao(view, cam, p, n)
        assert (np.ascontiguousarray(feat[..., 7]).view(np.uint32) != 0).all()  # every centre ray hits
        assert (clear.astype(F) / F(n) == ao).all()
        pw, got = want[floor], ao[floor].astype(np.float64)
        var = pw * (1 - pw)
        ok, zs = A.accept(got, pw, var, n, 2.0 ** -24)
        ok_all, z_all = A.accept(got.mean(), pw.mean(), var.mean(), n * floor.sum(), 2.0 ** -24)
        print(f"ao {'bvh' if bvh else 'list'} {reduction} {tn}: largest z {zs.max():.2f}, together {float(z_all):.2f}")
        assert ok.all() and ok_all
    # a radius below the gap between the floor and the sphere (h - r = 0.4): no ray from the floor is
    # occluded, exactly.  (On the sphere's own pixels a direction N + r of almost no length rounds to
    # one that points inwards, about once in 10^5 rays: the definition's f32, not held here.)
    ao, clear, _ = z.render_ao(view, cam, z.RenderParams(16, 16, 1, 4, bounded_volume_hierarchy=bvh), n, radius=0.3)
    assert (clear[floor] == n).all() and (ao[floor] == 1.0).all()


def test_ao_miss_pixels_keep_their_value():
    """FRAME_POSE over (e): the sky pixels beside the sphere miss - clear = n, ao = 1, whatever the
    radius - and a radius below the gap clears every floor pixel too."""
    c = A.cases()["occluded-floor"]
    _, view = c.scene(False)
    cam = z.camera_init(*AF.FRAME_POSE)
    floor = ~np.isnan(AF.ao_expected(cam, 16, 16, A.FLOOR, np.array(c.spheres[0][0]), A.OCC_R))
    for radius in (float("inf"), 0.3):
        ao, clear, feat = z.render_ao(view, cam, z.RenderParams(16, 16, 1, 4, bounded_volume_hierarchy=False), 100, radius=radius)
        miss = np.ascontiguousarray(feat[..., 7]).view(np.uint32) == 0
        assert miss[10:].all() and miss.sum() >= 100 and not (miss & floor).any() and floor.sum() >= 80
        assert (clear[miss] == 100).all() and (ao[miss] == 1.0).all()
    assert (clear[floor] == 100).all() and (ao[floor] == 1.0).all()  # (the last call: radius 0.3)


# ---- 6. the far end of the sample and ray fields ------------------------------------------

@pytest.mark.parametrize("first_sample,first_ray", [(65536 - SPP, 0), (0, (1 << 48) - N_RAYS), (65536 - SPP, (1 << 48) - N_RAYS)],
                         ids=["last-samples", "last-rays", "both"])
@pytest.mark.parametrize("name", ["lambert-sphere-generic-d2", "glass-0.6667-generic-d50"])
def test_far_end_of_the_key_fields(name, first_sample, first_ray):
    """Samples 65280 .. 65535 and rays 2^48 - 4096 .. 2^48 - 1: a key that wrapped or truncated
    would repeat streams, and 4096 x 256 samples would not average as independent ones."""
    c = A.cases()[name]
    _, view = c.scene(True)
    for prng in PRNGS.values():
        p = rparams(c, True, prng)
        ctx = z.RenderContext(view, p)
        try:
            mean, info = query(ctx, p, name, first_sample, first_ray)
            base, _ = query(ctx, p, name)
        finally:
            ctx.close()
        assert info["samples"] == N and (mean != base).any()
        check_mean(c, mean, N, f"{name} first_sample {first_sample} first_ray {first_ray}")
        T.check_counters(c, info, N, name)

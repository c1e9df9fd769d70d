"""CPU tests: the oracle against the closed forms of tests/analytic_ref.py (rays) and
tests/analytic_frames.py (frames), and proof that the comparison has power.  No kernel is
launched.

Every ray case runs through oracle_render in counter mode on the degenerate camera of
radiance_ref.ray_camera: a 64 x 64 frame of 256 samples per pixel is 4096 independent streams
along one ray, N = 2^20 samples (the 50-deep closed sphere: 16 x 16, N = 2^16), on the surface
list and - where the case has one - BVH-padded, under both PRNGs.  Pixel means are averaged in
float64 and held to

    |mean - expected| <= 5 sqrt(var / N) + floor        per channel,

var the closed-form single-sample variance, floor = (chunk + n_chunks + 2) 2^-24 the f32
rounding of the oracle's chunked sum.  Streams are seeded: a pass is reproducible.  A failure
is examined by running the case once more with four times the streams (a larger frame): a
deviation that keeps its absolute size is a bias, one that halves was chance (see
profiles/r20/analytic/README.md for the record).
"""
import functools

import numpy as np
import pytest

import analytic_frames as AF
import analytic_ref as A
import radiance_ref as R
import zraytrace_amd as z
from oracle import oracle_py as O

PRNGS = {"xoroshiro": z.ZRT_PRNG_XOROSHIRO128, "xoshiro": z.ZRT_PRNG_XOSHIRO256}
SPP = 256
_STATS = {"rays": "rays_processed", "reflections": "reflections", "background_hits": "background_hits",
          "recursion_depth_hits": "recursion_depth_hits"}
# What f32 geometry costs a case without variance: |oracle - float64| per channel, the largest
# over list / BVH and both PRNGs, measured once on the CPU.  The assertion allows four times it
# on top of the floor (2.5e-6 at 256 samples in chunks of 32).  Cases that are black are exact.
F32_COST = {"metal-sphere": 2.39e-7, "lambert-triangle-back": 2.49e-7, "glass-1.0-centre-d50": 3.98e-7,
            "periscope-d4": 1.74e-7, "glass-0.6667-grazing-d50": 4.94e-8}
VARIANTS = [(name, bvh) for name, c in A.cases().items() for bvh in ((False, True) if c.pad else (False,))]
IDS = [f"{n}-{'bvh' if b else 'list'}" for n, b in VARIANTS]


def margin(case, spp=SPP):
    """The rule's floor for a case: the chunked sum's rounding, what the closed form leaves out
    by a stated bound (extra_floor), and for a case without variance four times F32_COST."""
    return A.chunk_floor(spp) + case.extra_floor + 4.0 * F32_COST.get(case.name, 0.0)


@functools.lru_cache(maxsize=None)
def oracle_run(name, bvh, prng):
    """(mean colour float64[3], counters per sample, N) of a case through oracle_render."""
    c = A.cases()[name]
    _, view = c.scene(bvh)
    p = z.RenderParams(c.cpu_side, c.cpu_side, SPP, c.depth, bounded_volume_hierarchy=bvh, prng=prng)
    img, st = O.render(view, R.ray_camera(c.o, c.tgt), p)
    n = c.cpu_side * c.cpu_side * SPP
    assert st["samples_processed"] == n and st["used_bvh"] == int(bvh)
    return img.astype(np.float64).reshape(-1, 3).mean(0), {k: st[v] for k, v in _STATS.items()}, n


def check_counters(case, got, n, what):
    """Counts that have no variance with ==, the others by the rule (no floor: integers)."""
    for k in A.COUNTERS:
        if case.exact_counters or not case.counter_var[k]:
            assert got[k] == round(case.counters[k] * n), f"{what}: {k} {got[k]} != {case.counters[k]} N"
        else:
            ok, zs = A.accept(got[k] / n, case.counters[k], case.counter_var[k], n, 0.0)
            print(f"{what}: {k} {got[k] / n:.6f} expected {case.counters[k]:.6f} z {float(zs):.2f}")
            assert ok, f"{what}: {k} {got[k] / n} against {case.counters[k]}, z {float(zs):.2f}"
    # every path ends on the sky, at the depth limit or (metal only) absorbed; every ray but the last scatters
    assert got["rays"] == got["reflections"] + got["background_hits"]


@pytest.mark.parametrize("prng", list(PRNGS))
@pytest.mark.parametrize("name,bvh", VARIANTS, ids=IDS)
def test_oracle_meets_the_closed_form(name, bvh, prng):
    c = A.cases()[name]
    mean, counters, n = oracle_run(name, bvh, PRNGS[prng])
    ok, zs = A.accept(mean, c.mean(), c.var, n, margin(c))
    print(f"{name} {'bvh' if bvh else 'list'} {prng}: N {n} mean {mean} expected {c.mean()} "
          f"dev {np.abs(mean - c.mean()).max():.3e} z {zs.max():.2f}")
    assert ok.all(), f"{name}: mean {mean} against {c.mean()}, z {zs}"
    if c.counters is not None:
        check_counters(c, counters, n, name)


def test_the_cases_cover_what_they_name():
    """The case list holds what the anchors are for: four Lambertian normals, every ior at three
    impact parameters and depths 1, 2, 3, 50, a first hit that cannot refract, internal
    reflections, the closed sphere at 1, 5, 50, both periscope depths, padded variants of (a),
    (c), (d) and (e)."""
    cs = A.cases()
    assert len([n for n in cs if n.startswith("lambert-sphere") and n.endswith("-d2")]) == 4
    for ior in (1.5, 1.0, 2.4, 0.6667):
        mine = [g for g in A.GLASS if g[0] == ior]
        assert {"generic", "grazing"} <= {g[1] for g in mine} and {g[1] for g in mine} & {"centre", "near-centre"}
    assert {g[2] for g in A.GLASS} == {1, 2, 3, 50}
    tir = cs["glass-0.6667-grazing-d50"]
    assert tir.zero_variance and tir.counters["rays"] == 2  # reflected at the first, front hit: cannot_refract
    deep = A.dielectric_walk(*A._ray64(cs["glass-0.6667-generic-d50"].o, cs["glass-0.6667-generic-d50"].tgt),
                             float(np.float32(0.6667)), 50)
    assert len(deep) > 40 and sum(l[0] for l in deep if l[2][0] > 4) > 0.01  # the series has many terms
    assert cs["glass-1.0-centre-d50"].zero_variance
    for k in ("lambert-sphere", "glass", "closed-sphere", "occluded-floor", "metal"):
        assert any(c.pad for n, c in cs.items() if n.startswith(k)), k
    # the straight-below form of the issue is the general one at n = +y
    a, b, s2 = A.SKY_A, A.SKY_B, A.OCC_R ** 2 / A.OCC_H ** 2
    want = np.array(A.RHO) * (a + 2 / 3 * b - (a * s2 + 2 / 3 * b * (1 - (1 - s2) ** 1.5)))
    assert np.abs(cs["occluded-floor"].mean() - want).max() < 2e-7
    # the lobe's moments against a float64 quadrature of the density cos(theta) / pi
    c_, ph = np.meshgrid((np.arange(4000) + 0.5) / 4000, (np.arange(64) + 0.5) / 64 * 2 * np.pi, indexing="ij")
    for ny, cut in ((1.0, 1.0), (0.6, 1.0), (-0.8, 0.7), (0.0, 0.8)):
        dy = c_ * ny + np.sqrt(1 - c_ * c_) * np.cos(ph) * np.sqrt(1 - ny * ny)
        w = 2 * c_ * (c_ < cut)
        num = [(w * f).mean() for f in (np.ones_like(dy), dy, dy * dy)]
        assert np.allclose(num, A.lambert_moments(ny, cut), atol=2e-4)


# ---- f. frames through a real camera ------------------------------------------------------

FRAME_SPP = 1024


@functools.lru_cache(maxsize=None)
def frame_setup():
    cam = z.camera_init(*AF.FRAME_POSE)
    return cam, AF.classify_pixels(cam, z.ZRT_LENS_PINHOLE)


@functools.lru_cache(maxsize=None)
def oracle_frame(prng):
    cam, _ = frame_setup()
    _, view = AF.floor_scene()
    p = z.RenderParams(AF.FRAME_W, AF.FRAME_H, FRAME_SPP, 4, prng=prng)
    return O.render(view, cam, p)[0].astype(np.float64)


def check_frame(img, cls, lens, n, what, sky_model=None, floor_model=None, floor_ny=1.0):
    """Every classified pixel by the rule - floor pixels (1) against rho sky((2/3) n_y), sky
    pixels (2) of a pinhole `lens` against the quadrature; lens None: left out - and the floor
    pixels' mean together (N = pixels x n).  Returns (what fails, largest z)."""
    fm = A.lambert_mean_var(A.RHO, floor_ny, model=floor_model)[0]
    fv = A.lambert_mean_var(A.RHO, floor_ny)[1]
    bad, zmax, fl = [], 0.0, A.chunk_floor(n)
    for y, x in zip(*np.nonzero(cls)):
        if cls[y, x] == 1:
            m, v = fm, fv
        elif lens is None:
            continue
        else:
            m, v = AF.sky_pixel(lens, x, y, model=sky_model)[0], AF.sky_pixel(lens, x, y)[1]
        ok, zs = A.accept(img[y, x], m, v, n, fl)
        zmax = max(zmax, float(zs.max()))
        if not ok.all():
            bad.append((int(x), int(y), img[y, x], m))
    k = int((cls == 1).sum())
    if k:
        ok, zs = A.accept(img[cls == 1].mean(0), fm, fv, n * k, fl)
        zmax = max(zmax, float(zs.max()))
        if not ok.all():
            bad.append(("floor pixels together", k, img[cls == 1].mean(0), fm))
    print(f"{what}: {k} floor pixels, {int((cls == 2).sum())} sky pixels, largest z {zmax:.2f}")
    return bad, zmax


def test_frame_rows_are_what_they_are_named():
    """Rows 0 - 5 lie wholly on the floor, rows 8 - 15 wholly on the sky; the horizon crosses
    row 7 and the floor's far edge row 6: HORIZON_ROWS, left out."""
    _, cls = frame_setup()
    assert (cls[list(AF.FLOOR_ROWS)] == 1).all() and (cls[list(AF.SKY_ROWS)] == 2).all()
    assert not (cls[list(AF.HORIZON_ROWS)] == 1).any() and not (cls[7] == 2).all()


@pytest.mark.parametrize("prng", list(PRNGS))
def test_oracle_frame_meets_the_closed_forms(prng):
    cam, cls = frame_setup()
    bad, _ = check_frame(oracle_frame(PRNGS[prng]), cls, cam, FRAME_SPP, f"oracle frame {prng}")
    assert not bad, bad


# ---- power ----------------------------------------------------------------------------------

def rejecting_cases(model):
    """The (case, variant, prng) runs of this file whose oracle result the wrong model fails."""
    out = []
    for name, bvh in VARIANTS:
        c = A.cases()[name]
        for prng in PRNGS.values():
            mean, counters, n = oracle_run(name, bvh, prng)
            ok, _ = A.accept(mean, c.mean(model), c.var, n, margin(c))
            cnt_ok = True
            if c.counters_of is not None:
                cnt_ok = all(abs(counters[k] / n - v) <= 5 * np.sqrt(c.counter_var[k] / n)
                             for k, v in c.counters_of(model).items())
            if not (ok.all() and cnt_ok):
                out.append((name, bvh, prng))
    return out


@pytest.mark.parametrize("model", A.MODELS)
def test_a_wrong_model_is_rejected(model):
    """Each named wrong model fails the same rule at the same sample counts on at least one
    case - and the right model on none (test_oracle_meets_the_closed_form)."""
    if model == "jitter-0-1":
        cam, cls = frame_setup()
        bad, _ = check_frame(oracle_frame(PRNGS["xoroshiro"]), cls, cam, FRAME_SPP, model, sky_model=model)
        assert len(bad) >= 64, "a jitter range of [0, 1) passes on the sky rows"
        return
    got = rejecting_cases(model)
    print(f"{model}: rejected by {sorted({g[0] for g in got})}")
    assert got, f"no case rejects the wrong model {model}"
    want = {"uniform-hemisphere": "lambert", "r0-squared": "glass", "eta-swapped": "glass",
            "no-occluder": "occluded-floor"}.get(model)
    if want:
        assert all(w in " ".join(g[0] for g in got) for w in [want])
        if model == "uniform-hemisphere":  # every Lambertian case whose normal has a y component
            names = {g[0] for g in got}
            assert {"lambert-sphere-up-d2", "lambert-sphere-down-ish-d2", "lambert-triangle-front"} <= names


def test_the_floor_frame_rejects_a_uniform_hemisphere():
    cam, cls = frame_setup()
    bad, _ = check_frame(oracle_frame(PRNGS["xoroshiro"]), cls, None, FRAME_SPP, "uniform", floor_model="uniform-hemisphere")
    assert bad

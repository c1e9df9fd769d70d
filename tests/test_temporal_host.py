"""Host-side tests of the temporal accumulation (no GPU): the new entry points and their
ctypes signatures, zrt_debug_reproject_plan against the numpy f32 restatement, the defaults,
every refusal of zrt_ctx_temporal and zrt_render_temporal that needs no device, and the
properties of the restatement (tests/temporal_ref.py) that the GPU tests compare the kernel
against."""
import ctypes as C
import json
import math
import os
import re

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi

import shading_scenes as S
import temporal_ref as T
import test_denoise_guided_host as H

F = np.float32
NEW = ["zrt_debug_reproject_plan", "zrt_temporal_defaults", "zrt_ctx_temporal", "zrt_ctx_temporal_reset",
       "zrt_ctx_temporal_ms", "zrt_render_temporal"]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the interface ----------------------------------------------------------------------

def test_new_symbols_are_exported_and_bound():
    src = open(os.path.join(z.REPO, "include", "zrt.h")).read()
    declared = set(re.findall(r"\b(zrt_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    table = {name for name, _, _ in _ffi.SIGNATURES}
    for name in NEW:
        assert name in declared and name in table, name
        assert getattr(z.lib(), name).argtypes is not None
    assert "#define ZRT_ABI_VERSION 2" in src and z.lib().zrt_abi_version() == 2
    assert "ZRT_TA_DEMODULATE = 1u" in src and z.ZRT_TA_DEMODULATE == 1 == T.DEMODULATE
    assert f"ZRT_DEFAULT_TEMPORAL_HISTORY = {T.DEFAULT_HISTORY}u" in src
    assert C.sizeof(_ffi.ReprojectPlan) == 56 and C.sizeof(_ffi.Temporal) == 32


def test_temporal_defaults_are_legal_and_the_probes_winner():
    d = z.temporal_defaults()
    with open(os.path.join(z.REPO, "profiles", "r12", "temporal", "defaults.json")) as f:
        rec = json.load(f)
    for k in ("alpha_min", "max_history", "sigma_normal", "sigma_depth", "flags"):
        assert getattr(d, k) == rec["winner"][k], k
    assert 0.0 <= d.alpha_min <= 1.0
    assert 1 <= d.max_history <= 65535
    for k in ("sigma_normal", "sigma_depth"):
        assert math.isfinite(getattr(d, k)) and getattr(d, k) >= 0.0, k
    assert d.flags in (0, z.ZRT_TA_DEMODULATE) and list(d.reserved) == [0, 0, 0]


# ---- zrt_debug_reproject_plan -------------------------------------------------------------

def camera(look_from, look_at, vup=(0.0, 1.0, 0.0), vfov=40.0, aspect=1.0):
    cam = _ffi.Camera()
    f3 = C.c_float * 3
    _ffi.check(z.lib().zrt_camera_init(f3(*look_from), f3(*look_at), f3(*vup), vfov, aspect, C.byref(cam)))
    return cam


def assert_plan(cam, valid=None):
    got = z.debug_reproject_plan(T.cam_struct(cam), z.RenderParams(64, 64, 1, 1))
    want = T.reproject_plan(cam)
    for k in ("origin", "rn", "ru", "rv"):
        g = np.array([getattr(getattr(got, k), c) for c in "xyz"], F)
        same = (bits(g) == bits(want[k])) | (np.isnan(g) & np.isnan(want[k]))
        assert same.all(), (k, g, want[k])
    assert bits(F(got.s)) == bits(want["s"]) or (math.isnan(got.s) and np.isnan(want["s"]))
    assert bool(got.valid) == want["valid"]
    if valid is not None:
        assert bool(got.valid) == valid
    return want


SCENE_CAMERAS = [("scene", i) for i in (0, 1, 2, 3, 4)] + [("shading", n) for n in S.NAMES]


@pytest.mark.parametrize("kind,key", SCENE_CAMERAS, ids=[str(k) for _, k in SCENE_CAMERAS])
def test_reproject_plan_of_the_scenes_cameras(scenes, kind, key):
    """Whatever the sign of s, after the sign rule the plan maps the camera's own pixel-centre
    rays, at any depth, back to their pixels with den > 0."""
    cam = T.cam_array(scenes(key).camera if kind == "scene" else S.get(key)[2])
    plan = assert_plan(cam, valid=True)
    o, llc, Hh, W = cam
    rng = np.random.default_rng(5)
    x = np.arange(64, dtype=F)[None, :].repeat(64, 0)
    y = np.arange(64, dtype=F)[:, None].repeat(64, 1)
    e = ((llc + Hh * (x / F(64))[..., None]) + W * (y / F(64))[..., None]) - o
    dirn = e / np.sqrt((e * e).sum(-1, dtype=F))[..., None]
    d = (o + dirn * (rng.random((64, 64, 1), dtype=F) * F(20.0) + F(0.5))) - plan["origin"]
    den = T._dot(d, plan["rn"])
    assert (den > 0).all()
    fx, fy = (T._dot(d, plan["ru"]) / den) * F(64), (T._dot(d, plan["rv"]) / den) * F(64)
    assert np.abs(fx - x).max() <= 1e-3 and np.abs(fy - y).max() <= 1e-3


def test_reproject_plan_left_handed_and_degenerate():
    cam = T.cam_array(camera((1.0, 2.0, 5.0), (0.0, 0.5, 0.0), vfov=35.0, aspect=1.5))
    right = assert_plan(cam, valid=True)
    left = cam.copy()
    left[1] = cam[1] + cam[2]  # mirrored: the corner moves to the other side, horizontal flips
    left[2] = -cam[2]
    lp = assert_plan(left, valid=True)
    assert (right["s"] < 0) != (lp["s"] < 0)
    for c in (right, lp):  # after the sign rule both look forward: the centre of the view has den > 0
        o, llc, Hh, W = cam if c is right else left
        centre = (llc + Hh * F(0.5) + W * F(0.5)) - o
        assert T._dot(centre, c["rn"]) > 0
    par = cam.copy()
    par[3] = par[2] * F(0.5)  # horizontal parallel to vertical: rn = 0
    assert_plan(par, valid=False)
    flat = cam.copy()
    flat[1] = flat[0]  # the image plane through the origin: b = 0
    assert_plan(flat, valid=False)
    for row in range(4):
        bad = cam.copy()
        bad[row, 1] = np.nan
        assert_plan(bad, valid=False)
    with pytest.raises(z.ZrtError) as e:
        z.debug_reproject_plan(T.cam_struct(cam), z.RenderParams(8, 9, 1, 1))
    assert e.value.code == _ffi.ZRT_E_INVALID


# ---- refusals that need no device -----------------------------------------------------------

def _temporal_rc(width=8, height=8, frame=0x1000, feat=0x2000, var=0x3000, out=0x4000, out_var=0x5000,
                 out_len=0x6000, **fields):
    """zrt_ctx_temporal with no context: what it refuses of its arguments comes first."""
    tp = _ffi.Temporal(alpha_min=0.1, max_history=8, sigma_normal=1.0, sigma_depth=1.0, flags=0)
    for k, v in fields.items():
        setattr(tp, k, v)
    p = z.RenderParams(width, height, 1, 1).abi()
    cam = S.get("bubbles")[2]
    rc = z.lib().zrt_ctx_temporal(None, C.byref(cam), C.byref(p), C.byref(tp), C.c_void_p(frame), C.c_void_p(feat),
                                  C.c_void_p(var), C.c_void_p(out), C.c_void_p(out_var), C.c_void_p(out_len), None)
    return rc, z.lib().zrt_last_error().decode()


@pytest.mark.parametrize("field", ["sigma_normal", "sigma_depth"])
@pytest.mark.parametrize("value", [-1.0, float("nan"), float("inf")])
def test_temporal_bad_sigma_is_refused(field, value):
    rc, msg = _temporal_rc(**{field: value})
    assert rc == _ffi.ZRT_E_INVALID and field in msg


def test_temporal_other_refusals():
    for kw, word in (({"alpha_min": -0.01}, "alpha_min"), ({"alpha_min": 1.5}, "alpha_min"),
                     ({"alpha_min": float("nan")}, "alpha_min"), ({"max_history": 65536}, "max_history"),
                     ({"flags": 2}, "unknown flag"), ({"width": 8, "height": 9}, "height > width"),
                     ({"out": 0x1000}, "dev_out must not be dev_frame"), ({"feat": 0x2004}, "aligned"),
                     ({"var": None}, "dev_variance is null"), ({"out_var": 0x3000}, "dev_out_variance must not")):
        rc, msg = _temporal_rc(**kw)
        assert rc == _ffi.ZRT_E_INVALID and word in msg, (kw, msg)
    # what is valid gets as far as the missing context
    for kw in ({"alpha_min": 0.0, "max_history": 0}, {"alpha_min": 1.0, "max_history": 65535, "flags": 1},
               {"sigma_normal": 0.0, "sigma_depth": 0.0}, {"out_var": None, "out_len": None}):
        rc, msg = _temporal_rc(**kw)
        assert rc == _ffi.ZRT_E_INVALID and msg == "null argument", (kw, msg)
    assert z.lib().zrt_ctx_temporal_reset(None) == _ffi.ZRT_E_INVALID
    assert z.lib().zrt_ctx_temporal_ms(None, None) == _ffi.ZRT_E_INVALID


def test_render_temporal_refuses_before_any_device_work():
    """ZRT_E_INVALID also on a machine with no GPU, where a valid call would end in
    ZRT_E_NODEVICE: the guided one-shot's chunk rule, no frames, a bad temporal step or filter."""
    _, view, cam = S.get("bubbles")
    ok = z.RenderParams(8, 8, 8, 1, sample_chunk=4)
    for spp, chunk in ((10, 4), (4, 4), (32, 0), (24, 16)):
        with pytest.raises(z.ZrtError) as e:
            z.render_temporal(view, [cam, cam], z.RenderParams(8, 8, spp, 1, sample_chunk=chunk))
        assert e.value.code == _ffi.ZRT_E_INVALID and "sample_chunk" in str(e.value), (spp, chunk)
    with pytest.raises(z.ZrtError) as e:
        z.render_temporal(view, [], ok)
    assert e.value.code == _ffi.ZRT_E_INVALID and "n_frames" in str(e.value)
    with pytest.raises(z.ZrtError) as e:
        z.render_temporal(view, [cam], ok, temporal=_ffi.Temporal(alpha_min=2.0))
    assert e.value.code == _ffi.ZRT_E_INVALID and "alpha_min" in str(e.value)
    with pytest.raises(z.ZrtError) as e:
        z.render_temporal(view, [cam], ok, denoise=_ffi.Denoise(iterations=9, sigma_color=1.0))
    assert e.value.code == _ffi.ZRT_E_INVALID
    with pytest.raises(z.ZrtError) as e:
        z.render_temporal(view, [cam], ok, flags=4)
    assert e.value.code == _ffi.ZRT_E_INVALID and "flag" in str(e.value)


# ---- the restatement ------------------------------------------------------------------------

def sequence(h, w, seed, frames):
    """Frames of H.synthetic sharing one feature buffer: seeded colours and variances."""
    _, feat, _ = H.synthetic(h, w, seed)
    out = []
    for k in range(frames):
        frame, _, var = H.synthetic(h, w, seed + 100 * (k + 1))
        out.append((frame, var))
    return feat, out


@pytest.mark.parametrize("flags", [0, T.DEMODULATE], ids=["plain", "demodulated"])
def test_static_camera_is_the_running_mean(flags):
    """A static camera, alpha_min 0, max_history >= N: one tap of weight 1 survives, so frame
    N's output is the recursion h (1 - 1/n) + c (1/n) bit for bit, the variance the same with
    squared weights, and len = N on every hit pixel of D (1 on misses, 0 outside D)."""
    h, w, N = 13, 14, 5
    cam = T.cam_array(S.get("bubbles")[2])
    feat, seq = sequence(h, w, 3, N)
    hit = np.ascontiguousarray(feat[:, :h, 7]).view(np.uint32) != 0
    assert hit.any() and not hit.all()
    t = T.Temporal()
    mean = mvar = None
    for k, (frame, var) in enumerate(seq):
        n = k + 1
        got, gv, gl = t.step(cam, frame, feat, var, 0.0, N + 3, 0.25, 0.25, flags)
        c, v = frame[:, :h].copy(), var[:, :h].copy()
        if flags:
            alb = feat[:, :h, 4:7]
            big = hit[..., None] & (alb > T.A_MIN)
            c = np.where(big, c / alb, c).astype(F)
            am = ((alb[..., 0] + alb[..., 1]) + alb[..., 2]) * (F(1.0) / F(3.0))
            vbig = hit & (am > T.A_MIN)
            v = np.where(vbig, v / (am * am), v).astype(F)
        if k == 0:
            mean, mvar = c, v
        else:
            al = F(1.0) / F(n)
            om = F(1.0) - al
            mean = np.where(hit[..., None], mean * om + c * al, c)
            mvar = np.where(hit, mvar * (om * om) + v * (al * al), v)
        want, wv = mean, mvar
        if flags:
            want = np.where(big, want * alb, want).astype(F)
            wv = np.where(vbig, wv * (am * am), wv).astype(F)
        assert (bits(got[:, :h]) == bits(want)).all() and (bits(gv[:, :h]) == bits(wv)).all(), n
        assert (gl[:, :h][hit] == n).all() and (gl[:, :h][~hit] == 1).all() and (gl[:, h:] == 0).all()
        assert (got[:, h:] == frame[:, h:]).all() and (gv[:, h:] == var[:, h:]).all()
        assert t.last["static"] == (k > 0) and t.last["blended"] == (hit.sum() if k else 0)


def test_max_history_one_and_alpha_one_pass_the_input_through():
    """n = 1: r = 1, al = 1, om = 0, out = h * 0 + c * 1 = c for a finite history."""
    cam = T.cam_array(S.get("bubbles")[2])
    feat, seq = sequence(12, 12, 8, 3)
    for kw in (dict(alpha_min=0.0, max_history=1), dict(alpha_min=1.0, max_history=9)):
        t = T.Temporal()
        for frame, var in seq:
            got, gv, gl = t.step(cam, frame, feat, var, kw["alpha_min"], kw["max_history"], 0.0, 0.0)
            assert (bits(got) == bits(frame)).all() and (bits(gv) == bits(var)).all()
            if kw["max_history"] == 1:
                assert gl.max() == 1


def test_reset_size_flag_and_invalid_plan_drop_the_history():
    cam = T.cam_array(S.get("bubbles")[2])
    feat, seq = sequence(12, 12, 9, 2)
    (f0, v0), (f1, v1) = seq
    t = T.Temporal()
    t.step(cam, f0, feat, v0, 0.0, 8, 0.0, 0.0)
    got, _, gl = t.step(cam, f1, feat, v1, 0.0, 8, 0.0, 0.0)
    assert gl.max() == 2 and (got != f1).any()
    for how in ("reset", "size", "flag", "plan"):
        t = T.Temporal()
        c0 = cam.copy()
        if how == "plan":
            c0[3] = c0[2]
        if how == "size":
            f, s = sequence(10, 12, 9, 1)
            t.step(c0, s[0][0], f, s[0][1], 0.0, 8, 0.0, 0.0)
        else:
            t.step(c0, f0, feat, v0, 0.0, 8, 0.0, 0.0, T.DEMODULATE if how == "flag" else 0)
        if how == "reset":
            t.reset()
        got, gv, gl = t.step(cam, f1, feat, v1, 0.0, 8, 0.0, 0.0)
        assert (bits(got) == bits(f1)).all() and (bits(gv) == bits(v1)).all() and gl.max() == 1, how
        assert not t.last["history"]


def test_nan_pixel_does_not_outlive_one_frame():
    cam = T.cam_array(S.get("bubbles")[2])
    feat, seq = sequence(12, 12, 10, 3)
    t = T.Temporal()
    t.step(cam, seq[0][0], feat, seq[0][1], 0.0, 8, 0.25, 0.25)
    f1 = seq[1][0].copy()
    f1[4, 5, 1] = np.nan
    got, gv, gl = t.step(cam, f1, feat, seq[1][1], 0.0, 8, 0.25, 0.25)
    assert np.isnan(got[4, 5, 1]) and np.isnan(got).sum() == 1 and not np.isnan(gv).any() and gl[4, 5] == 2
    got, gv, gl = t.step(cam, seq[2][0], feat, seq[2][1], 0.0, 8, 0.25, 0.25)
    assert not np.isnan(got).any() and gl[4, 5] == 1 and t.last["rejected_nan"] == 1
    assert (bits(got[4, 5]) == bits(seq[2][0][4, 5])).all() and gl[4, 6] == 3

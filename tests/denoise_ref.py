"""Restatements for the denoiser's tests (test infrastructure).

  atrous()             the edge-avoiding a-trous filter of include/zrt.h "denoising" in
                       numpy, f32 operation by operation in the definition's order: what
                       zrt_ctx_denoise must return bit for bit.
  expected_features()  the first-hit feature buffer of a frame composed from the oracle
                       alone: the pixel-centre ray in camera_get_ray's operation order,
                       O.trace for the primitive and t, O.sphere_hit / O.triangle_hit for
                       the hit record's normal, O.texture_albedo for image textures; only
                       a triangle's (u, v), which oracle_triangle_hit does not return,
                       is restated here (triangle_uv; tests/test_denoise_host.py checks it
                       against the location the oracle reports).
"""
import numpy as np

from zraytrace_amd import _ffi

F = np.float32
H5 = (F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625))  # h(-2 .. 2)
DEFAULT_ITERATIONS = 5


def _f32(*arrays):
    for a in arrays:
        assert a.dtype == np.float32, a.dtype


def _l1(d):
    """(|d.r| + |d.g|) + |d.b| in f32."""
    a = np.abs(d)
    _f32(a)
    return (a[..., 0] + a[..., 1]) + a[..., 2]


def atrous(frame, features, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth):
    """frame float32[H, W, 3], features float32[H, W, 8] -> the filtered frame.
    iterations 0 selects the default; a sigma of 0 switches its term off."""
    frame = np.ascontiguousarray(frame)
    features = np.ascontiguousarray(features)
    _f32(frame, features)
    height, width, _ = frame.shape
    assert features.shape == (height, width, 8) and height <= width
    n = height
    iterations = iterations or DEFAULT_ITERATIONS
    assert 1 <= iterations <= 8
    one = F(1.0)
    sig = [F(s) for s in (sigma_color, sigma_normal, sigma_albedo, sigma_depth)]
    on = [bool(s > 0) for s in sig]
    inv_c, inv_n, inv_a, inv_z = [one / s if o else F(0.0) for s, o in zip(sig, on)]
    col = frame[:, :n, :].copy()
    nrm = features[:, :n, 0:3]
    dep = features[:, :n, 3]
    alb = features[:, :n, 4:7]
    hit = np.ascontiguousarray(features[:, :n, 7]).view(np.uint32) != 0
    with np.errstate(all="ignore"):
        rz = np.where(hit, one / dep, F(0.0)).astype(F)
        kz = inv_z * rz
        _f32(rz, kz)
        for i in range(iterations):
            s = 1 << i
            kc = inv_c * F(1 << i)
            _f32(np.asarray(kc))
            acc = np.zeros_like(col)
            wsum = np.zeros((n, n), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    # the pixels p whose tap q = p + s (dx, dy) lies inside D
                    px0, px1 = max(0, -s * dx), min(n, n - s * dx)
                    py0, py1 = max(0, -s * dy), min(n, n - s * dy)
                    if px0 >= px1 or py0 >= py1:
                        continue
                    P = (slice(py0, py1), slice(px0, px1))
                    Q = (slice(py0 + s * dy, py1 + s * dy), slice(px0 + s * dx, px1 + s * dx))
                    if dx == 0 and dy == 0:
                        w = H5[2] * H5[2]
                        acc[P] = acc[P] + col[Q] * w
                        wsum[P] = wsum[P] + w
                        continue
                    ok = hit[P] == hit[Q]
                    w = np.full(ok.shape, H5[dx + 2] * H5[dy + 2], F)
                    if on[0]:
                        t = one - _l1(col[P] - col[Q]) * kc
                        ok &= t > 0
                        w = w * t
                    if on[1]:
                        d = nrm[P] - nrm[Q]
                        t = one - ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * inv_n
                        ok &= t > 0
                        w = w * t
                    if on[2]:
                        t = one - _l1(alb[P] - alb[Q]) * inv_a
                        ok &= t > 0
                        w = w * t
                    if on[3]:
                        t = one - np.abs(dep[P] - dep[Q]) * kz[P]
                        ok &= t > 0
                        w = w * t
                    _f32(w)
                    ok &= w > 0
                    acc[P] = np.where(ok[..., None], acc[P] + col[Q] * w[..., None], acc[P])
                    wsum[P] = np.where(ok, wsum[P] + w, wsum[P])
            _f32(acc, wsum)
            col = acc / wsum[..., None]
            _f32(col)
    out = frame.copy()
    out[:, :n, :] = col
    return out


def atrous_dn(frame, features, dn):
    """atrous() with the fields of a zrt_denoise (_ffi.Denoise)."""
    return atrous(frame, features, dn.iterations, dn.sigma_color, dn.sigma_normal, dn.sigma_albedo, dn.sigma_depth)


# ---- expected features, from the oracle ----------------------------------------------

def _v3(v):
    return np.array([v.x, v.y, v.z], F)


def pixel_rays(cam, width, height):
    """Pixel-centre primary rays (raytrace.zig:173-175 at r = 0.5: u = x / width,
    v = y / height; camera.zig:46-51: ((llc + hor u) + ver v) - origin) in f32:
    (origins[h, w, 3], raw directions[h, w, 3])."""
    o, llc, hor, ver = _v3(cam.origin), _v3(cam.lower_left_corner), _v3(cam.horizontal), _v3(cam.vertical)
    u = (np.arange(width, dtype=F) / F(width))[None, :, None]
    v = (np.arange(height, dtype=F) / F(height))[:, None, None]
    d = ((llc + hor * u) + ver * v) - o
    _f32(d)
    return np.broadcast_to(o, d.shape).copy(), d


def unit(d):
    """unitVector (vector.zig:88-92) in f32: each component divided by the length."""
    d = np.asarray(d, F)
    length = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    _f32(length)
    return d / length[..., None]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(p, q):
    return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]], F)


def triangle_uv(a, b, c, o, d_unit):
    """The barycentrics of oracle.c's triangle_hit (triangle.zig:48-60) in f32."""
    a, b, c, o, d = (np.asarray(x, F) for x in (a, b, c, o, d_unit))
    e1, e2 = b - a, c - a
    inv_det = F(1.0) / -_dot(d, _cross(e1, e2))
    dao = _cross(o - a, d)
    u, v = _dot(e2, dao) * inv_det, -_dot(e1, dao) * inv_det
    _f32(u, v)
    return u, v


def background(d_unit):
    """backgroundColor (raytrace.zig:52-60) of a ray whose direction Ray.init normalised."""
    y = unit(np.asarray(d_unit, F))[1]
    t = F(0.5) * (y + F(1.0))
    white = F(1.0) - t
    out = np.array([white + F(0.5) * t, white + F(0.7) * t, white + F(1.0) * t], F)
    return out


def _prim_vec(p, names):
    return [(getattr(p, k).x, getattr(p, k).y, getattr(p, k).z) for k in names]


def expected_features(O, scene, camera, width, height, bvh=True):
    """float32[height, width, 8] composed from the oracle; scene: a _ffi.Scene (or a
    pointer to one).  Also returns the list of (a, b, c, o, d_unit, u, v, location)
    of every image-textured triangle hit, for the check of triangle_uv."""
    s = scene.contents if hasattr(scene, "contents") else scene
    view = scene if hasattr(scene, "contents") else None
    if view is None:
        import ctypes as C
        view = C.pointer(s)
    out = np.zeros((height, width, 8), F)
    n = height
    o, d = pixel_rays(camera, width, height)
    o, d = o[:, :n].reshape(-1, 3), d[:, :n].reshape(-1, 3)
    use_bvh = bool(bvh) and s.n_prims > 10
    t, prim = O.trace(view, use_bvh, o, d)
    du = unit(d)
    inf = float("inf")
    tri_uv = []
    images = {}
    for k in range(len(d)):
        y, x = divmod(k, n)
        if prim[k] < 0:
            out[y, x, 4:7] = background(du[k])
            continue
        p = s.prims[int(prim[k])]
        m = s.materials[p.material]
        need_uv = m.kind != _ffi.ZRT_MAT_DIELECTRIC and s.textures[m.texture].kind == _ffi.ZRT_TEX_IMAGE
        if p.kind == _ffi.ZRT_PRIM_SPHERE:
            (center,) = _prim_vec(p, ("center",))
            ok, rec = O.sphere_hit(center, p.radius, o[k], d[k], 0.001, inf)
            u, v = rec[7], rec[8]
        else:
            a, b, c = _prim_vec(p, ("a", "b", "c"))
            ok, rec = O.triangle_hit(a, b, c, o[k], d[k], 0.001, inf)
            u = v = F(0.0)
            if need_uv:
                u, v = triangle_uv(a, b, c, o[k], du[k])
                tri_uv.append((a, b, c, o[k], du[k], u, v, rec[0:3].copy()))
        assert ok and rec[6] == t[k]
        out[y, x, 0:3] = rec[3:6]
        out[y, x, 3] = t[k]
        if m.kind == _ffi.ZRT_MAT_DIELECTRIC:
            out[y, x, 4:7] = 1.0
        else:
            tex = s.textures[m.texture]
            if tex.kind == _ffi.ZRT_TEX_IMAGE:
                if tex.image not in images:
                    im = s.images[tex.image]
                    images[tex.image] = np.ctypeslib.as_array(im.pixels, shape=(im.height, im.width, 3)).copy()
                out[y, x, 4:7] = O.texture_albedo(images[tex.image], tex.u_offset, tex.v_offset, float(u), float(v))
            else:
                out[y, x, 4:7] = (tex.color.x, tex.color.y, tex.color.z)
        out[y, x, 7:8] = np.array([int(prim[k]) + 1], np.uint32).view(F)
    return out, tri_uv

"""References for the post chain of lens frames (include/zrt.h "denoising lens frames").
Test infrastructure: used by tests/test_lens_post_host.py (CPU) and tests/test_gpu_lens_post.py.

  centre_rays()             the centre ray of every pixel of a rectangle: camera_ref.model at
                            (x / width, y / height), the thin lens taken as the pinhole.
  expected_lens_features()  the feature buffer along those rays composed from the oracle as
                            denoise_ref.expected_features composes the pinhole's: O.trace,
                            O.sphere_hit, O.triangle_hit, O.texture_albedo.
  moments()                 sum.rgb and Q of a camera query from camera_ref.Frame.cols, through
                            radiance_ref.chunk_sums and denoise_guided_ref.accumulate.
  atrous_rect(), guided_rect()  the two filters of zrt.h with a rectangle as their domain D, in
                            numpy, f32 operation by operation in the definitions' order.
"""
import ctypes as C

import numpy as np

import camera_ref as CR
import denoise_guided_ref as G
import denoise_ref as D
import radiance_ref as R
import zraytrace_amd as z
from denoise_ref import background, triangle_uv, unit
from zraytrace_amd import _ffi

F = np.float32


def _f32(*arrays):
    for a in arrays:
        assert np.asarray(a).dtype == np.float32, np.asarray(a).dtype


# ---- lens features -----------------------------------------------------------------------

def centre_rays(O, lens, p, rect):
    """(xs, ys, o float32[n, 3], d float32[n, 3]) over the rectangle's pixels, row-major from its
    bottom row: d = tgt - o, not normalised.  u = float(x) / float(width), v = float(y) /
    float(height): the camera query's jitter formula at r1 = r2 = 0.5."""
    xs, ys, _ = CR.pixels_of(p.width, rect)
    o = np.zeros((len(xs), 3), F)
    d = np.zeros((len(xs), 3), F)
    fw, fh = F(p.width), F(p.height)
    for i, (x, y) in enumerate(zip(xs, ys)):
        u, v = F(x) / fw, F(y) / fh
        assert ((F(x) + F(0.5)) - F(0.5)) / fw == u and ((F(y) + F(0.5)) - F(0.5)) / fh == v
        if lens.kind == z.ZRT_LENS_THIN:  # at its centre: the pinhole branch, no lens stream
            oo, tt = CR.vec(lens.origin), CR.plane_point(lens, u, v)
        else:
            oo, tt = CR.model(O, lens, u, v, 0, 0)
        o[i], d[i] = oo, (tt - oo).astype(F)
    return xs, ys, o, d


def _prim_vec(p, names):
    return [(getattr(p, k).x, getattr(p, k).y, getattr(p, k).z) for k in names]


def expected_lens_features(O, scene, lens, p, rect=None, bvh=True):
    """float32[height, width, 8]: the rectangle's pixels composed from the oracle, zero
    elsewhere.  scene: a pointer to a _ffi.Scene (or the struct)."""
    s = scene.contents if hasattr(scene, "contents") else scene
    view = scene if hasattr(scene, "contents") else C.pointer(s)
    rect = rect or (0, 0, p.width, p.height)
    out = np.zeros((p.height, p.width, 8), F)
    xs, ys, o, d = centre_rays(O, lens, p, rect)
    use_bvh = bool(bvh) and s.n_prims > 10
    t, prim = O.trace(view, use_bvh, o, d)
    du = unit(d)
    inf = float("inf")
    images = {}
    for k in range(len(d)):
        y, x = int(ys[k]), int(xs[k])
        if prim[k] < 0:
            out[y, x, 4:7] = background(du[k])
            continue
        pr = s.prims[int(prim[k])]
        m = s.materials[pr.material]
        need_uv = m.kind != _ffi.ZRT_MAT_DIELECTRIC and s.textures[m.texture].kind == _ffi.ZRT_TEX_IMAGE
        if pr.kind == _ffi.ZRT_PRIM_SPHERE:
            (center,) = _prim_vec(pr, ("center",))
            ok, rec = O.sphere_hit(center, pr.radius, o[k], d[k], 0.001, inf)
            u, v = rec[7], rec[8]
        else:
            a, b, c = _prim_vec(pr, ("a", "b", "c"))
            ok, rec = O.triangle_hit(a, b, c, o[k], d[k], 0.001, inf)
            u = v = F(0.0)
            if need_uv:
                u, v = triangle_uv(a, b, c, o[k], du[k])
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
    return out


# ---- moments and the variance plane ------------------------------------------------------

def moments(cols, chunk, sum0=None):
    """zrt_ctx_camera_moments' sum over the sample colours cols float32[n, k, 3] of one call
    (camera_ref.Frame.cols): float32[n, 4] = {sum.rgb, Q}.  Every chunk sum is
    radiance_ref.chunk_sums of the chunk's samples alone; the whole chunks go through
    denoise_guided_ref.accumulate, a ragged last chunk into the sums only.  sum0 (float32[n,
    4]): the sums and Q the call adds onto (ZRT_CQ_ACCUMULATE)."""
    n, k, _ = cols.shape
    c = chunk or 32
    out = np.zeros((n, 4), F) if sum0 is None else np.array(sum0, F)
    for j0 in range(0, k, c):
        s = R.chunk_sums(cols[:, j0:j0 + c], c)[:, :3]  # S_j: sequential from 0
        out[:, :3] = out[:, :3] + s
        if j0 + c <= k:
            _, q = G.accumulate(s.reshape(1, 1, n, 3))
            out[:, 3] = out[:, 3] + q[0]  # Q = Q + l_j * l_j (accumulate's own l * l from 0 is exact to add)
    _f32(out)
    return out


def variance_of(sums, chunk, n_total):
    """The plane values of {sum.rgb, Q} float32[n, 4] after n_total samples: denoise_guided_ref.variance."""
    c = chunk or 32
    assert n_total % c == 0 and n_total // c >= 2
    return G.variance(sums[:, :3], sums[:, 3], c, n_total // c)


# ---- the filters on a rectangle ----------------------------------------------------------

def _taps(ny, nx, s, dx, dy):
    """The pixels P of D = [0, ny) x [0, nx) whose tap Q = P + s (dx, dy) lies inside D, or None."""
    px0, px1 = max(0, -s * dx), min(nx, nx - s * dx)
    py0, py1 = max(0, -s * dy), min(ny, ny - s * dy)
    if px0 >= px1 or py0 >= py1:
        return None
    return ((slice(py0, py1), slice(px0, px1)),
            (slice(py0 + s * dy, py1 + s * dy), slice(px0 + s * dx, px1 + s * dx)))


def _setup(frame, features, rect, sigmas):
    frame = np.ascontiguousarray(frame)
    features = np.ascontiguousarray(features)
    _f32(frame, features)
    height, width, _ = frame.shape
    assert features.shape == (height, width, 8)
    x0, y0, w, h = rect
    assert w > 0 and h > 0 and x0 + w <= width and y0 + h <= height
    dom = (slice(y0, y0 + h), slice(x0, x0 + w))
    one = F(1.0)
    sig = [F(s) for s in sigmas]
    on = [bool(s > 0) for s in sig]
    inv = [one / s if o else F(0.0) for s, o in zip(sig, on)]
    feat = features[dom]
    hit = np.ascontiguousarray(feat[..., 7]).view(np.uint32) != 0
    return frame, dom, sig, on, inv, feat[..., 0:3], feat[..., 3], feat[..., 4:7], hit


def _geometry_terms(P, Q, w, ok, on, nrm, alb, dep, inv_n, inv_a, kz):
    one = F(1.0)
    if on[1]:
        d = nrm[P] - nrm[Q]
        t = one - ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * inv_n
        ok &= t > 0
        w = w * t
    if on[2]:
        t = one - D._l1(alb[P] - alb[Q]) * inv_a
        ok &= t > 0
        w = w * t
    if on[3]:
        t = one - np.abs(dep[P] - dep[Q]) * kz[P]
        ok &= t > 0
        w = w * t
    return w, ok


def atrous_rect(frame, features, rect, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth):
    """zrt.h "denoising" with D = rect = (x0, y0, w, h): frame float32[H, W, 3], features
    float32[H, W, 8] -> the filtered frame; pixels outside rect are copied."""
    frame, dom, sig, on, (inv_c, inv_n, inv_a, inv_z), nrm, dep, alb, hit = _setup(
        frame, features, rect, (sigma_color, sigma_normal, sigma_albedo, sigma_depth))
    iterations = iterations or D.DEFAULT_ITERATIONS
    assert 1 <= iterations <= 8
    one = F(1.0)
    col = frame[dom].copy()
    ny, nx = col.shape[:2]
    with np.errstate(all="ignore"):
        rz = np.where(hit, one / dep, F(0.0)).astype(F)
        kz = inv_z * rz
        _f32(rz, kz)
        for i in range(iterations):
            s = 1 << i
            kc = inv_c * F(1 << i)
            acc = np.zeros_like(col)
            wsum = np.zeros((ny, nx), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = _taps(ny, nx, s, dx, dy)
                    if pq is None:
                        continue
                    P, Q = pq
                    if dx == 0 and dy == 0:
                        w = D.H5[2] * D.H5[2]
                        acc[P] = acc[P] + col[Q] * w
                        wsum[P] = wsum[P] + w
                        continue
                    ok = hit[P] == hit[Q]
                    w = np.full(ok.shape, D.H5[dx + 2] * D.H5[dy + 2], F)
                    if on[0]:
                        t = one - D._l1(col[P] - col[Q]) * kc
                        ok &= t > 0
                        w = w * t
                    w, ok = _geometry_terms(P, Q, w, ok, on, nrm, alb, dep, inv_n, inv_a, kz)
                    _f32(w)
                    ok &= w > 0
                    acc[P] = np.where(ok[..., None], acc[P] + col[Q] * w[..., None], acc[P])
                    wsum[P] = np.where(ok, wsum[P] + w, wsum[P])
            _f32(acc, wsum)
            col = acc / wsum[..., None]
            _f32(col)
    out = frame.copy()
    out[dom] = col
    return out


def _smooth3(var):
    """g over a [ny, nx] domain: dy outer, dx inner, a neighbour outside D contributes the centre's value."""
    ny, nx = var.shape
    g = np.zeros_like(var)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            wt = G.W3[(dx == 0) + (dy == 0)]
            v = var.copy()
            pq = _taps(ny, nx, 1, dx, dy)
            if pq is not None:
                v[pq[0]] = var[pq[1]]
            g = g + v * wt
    _f32(g)
    return g


def guided_rect(frame, features, variance_plane, rect, iterations, sigma_color, sigma_normal, sigma_albedo,
                sigma_depth, flags=0):
    """zrt.h "variance-guided denoising" with D = rect: -> (the filtered frame, the filtered
    variance); pixels outside rect are copied in both."""
    variance_plane = np.ascontiguousarray(variance_plane)
    _f32(variance_plane)
    frame, dom, sig, on, (_, inv_n, inv_a, inv_z), nrm, dep, alb, hit = _setup(
        frame, features, rect, (sigma_color, sigma_normal, sigma_albedo, sigma_depth))
    assert variance_plane.shape == frame.shape[:2]
    iterations = iterations or D.DEFAULT_ITERATIONS
    assert 1 <= iterations <= 8
    one = F(1.0)
    col = frame[dom].copy()
    var = variance_plane[dom].copy()
    ny, nx = var.shape
    demod = bool(flags & G.DEMODULATE)
    with np.errstate(all="ignore"):
        if demod:
            big = hit[..., None] & (alb > G.A_MIN)
            col = np.where(big, col / alb, col).astype(F)
            am = ((alb[..., 0] + alb[..., 1]) + alb[..., 2]) * (one / F(3.0))
            vbig = hit & (am > G.A_MIN)
            var = np.where(vbig, var / (am * am), var).astype(F)
            _f32(am)
        rz = np.where(hit, one / dep, F(0.0)).astype(F)
        kz = inv_z * rz
        _f32(rz, kz, col, var)
        for i in range(iterations):
            s = 1 << i
            if on[0]:
                kl = one / (sig[0] * np.sqrt(_smooth3(var)) + F(2.0 ** -20))
                _f32(kl)
            lum = G._lum(col)
            acc = np.zeros_like(col)
            wsum = np.zeros((ny, nx), F)
            vacc = np.zeros((ny, nx), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    pq = _taps(ny, nx, s, dx, dy)
                    if pq is None:
                        continue
                    P, Q = pq
                    if dx == 0 and dy == 0:
                        w = D.H5[2] * D.H5[2]
                        acc[P] = acc[P] + col[Q] * w
                        wsum[P] = wsum[P] + w
                        vacc[P] = vacc[P] + var[Q] * (w * w)
                        continue
                    ok = hit[P] == hit[Q]
                    w = np.full(ok.shape, D.H5[dx + 2] * D.H5[dy + 2], F)
                    if on[0]:
                        t = one - np.abs(lum[P] - lum[Q]) * kl[P]
                        ok &= t > 0
                        w = w * t
                    w, ok = _geometry_terms(P, Q, w, ok, on, nrm, alb, dep, inv_n, inv_a, kz)
                    _f32(w)
                    ok &= w > 0
                    acc[P] = np.where(ok[..., None], acc[P] + col[Q] * w[..., None], acc[P])
                    wsum[P] = np.where(ok, wsum[P] + w, wsum[P])
                    vacc[P] = np.where(ok, vacc[P] + var[Q] * (w * w), vacc[P])
            _f32(acc, wsum, vacc)
            col = acc / wsum[..., None]
            var = vacc / (wsum * wsum)
            _f32(col, var)
        if demod:
            col = np.where(big, col * alb, col).astype(F)
            var = np.where(vbig, var * (am * am), var).astype(F)
    out = frame.copy()
    out[dom] = col
    out_var = variance_plane.copy()
    out_var[dom] = var
    return out, out_var


def atrous_rect_dn(frame, features, rect, dn):
    return atrous_rect(frame, features, rect, dn.iterations, dn.sigma_color, dn.sigma_normal, dn.sigma_albedo,
                       dn.sigma_depth)


def guided_rect_dn(frame, features, variance_plane, rect, dn, flags=0):
    return guided_rect(frame, features, variance_plane, rect, dn.iterations, dn.sigma_color, dn.sigma_normal,
                       dn.sigma_albedo, dn.sigma_depth, flags)

"""Restatements for the variance plane and the variance-guided filter (test infrastructure).

  chunk_sums()   the oracle's chunk sums of a frame: a render of samples_per_pixel = c with
                 the seed moved by j c phi^-1 (mod 2^64) draws chunk j's streams - the stream
                 key is ((pixel << 16) | s) + seed phi and phi is odd - and for a power-of-two
                 c its mean times c is the chunk sum bit for bit.
  accumulate()   include/zrt.h "the variance plane" in numpy: the sums and the second moment
                 Q of chunk sums added in order.
  variance()     ... and the plane from them, f32 operation by operation.
  guided()       include/zrt.h "variance-guided denoising" in numpy, in the definition's
                 order: what zrt_ctx_denoise_guided must return bit for bit.
"""
import dataclasses

import numpy as np

import denoise_ref as R

F = np.float32
PHI = 0x9E3779B97F4A7C15
PHI_INV = pow(PHI, -1, 1 << 64)
A_MIN = F(2.0 ** -6)
DEMODULATE = 1
W3 = (F(0.0625), F(0.125), F(0.25))  # 3 x 3 weights by the number of zero offsets


def _f32(*arrays):
    for a in arrays:
        assert np.asarray(a).dtype == np.float32, np.asarray(a).dtype


# ---- the variance plane -----------------------------------------------------------------

def chunk_sums(O, view, cam, p, k):
    """float32[k, H, W, 3]: the chunk sums 0 .. k - 1 of p's frame (p.sample_chunk a power of
    two), from the oracle alone."""
    c = p.sample_chunk
    assert c > 0 and c & (c - 1) == 0
    out = []
    for j in range(k):
        q = dataclasses.replace(p, samples_per_pixel=c, seed=(p.seed + j * c * PHI_INV) % (1 << 64),
                                rank=0, world_size=1, flags=0)
        img, _ = O.render(view, cam, q)
        s = img * F(c)
        _f32(s)
        out.append(s)
    return np.stack(out)


def accumulate(sums):
    """(acc float32[H, W, 3], Q float32[H, W]) of chunk sums float32[k, H, W, 3] added in order."""
    _f32(sums)
    acc = np.zeros(sums.shape[1:], F)
    q = np.zeros(sums.shape[1:3], F)
    for s in sums:
        acc = acc + s
        l = (s[..., 0] + s[..., 1]) + s[..., 2]
        q = q + l * l
    _f32(acc, q)
    return acc, q


def plan(c, k):
    """(ik, sc): the host's f32 scales."""
    ik = F(1.0) / F(k)
    sc = F(1.0) / (F(k - 1) * (F(c) * F(c)))
    _f32(ik, sc)
    return ik, sc


def variance(acc, q, c, k):
    """The plane of pixels holding k chunk sums of c samples."""
    ik, sc = plan(c, k)
    with np.errstate(all="ignore"):
        m = (acc[..., 0] + acc[..., 1]) + acc[..., 2]
        mean = m * ik
        v = q * ik - mean * mean
        v = np.where((v > 0) | np.isnan(v), v, F(0.0)).astype(F)
        var = v * sc
    _f32(var)
    return var


def frame_variance(sums, c, n):
    """The frame-layout plane float32[H, W] of a frame of height n: zero for x >= n."""
    acc, q = accumulate(sums)
    var = variance(acc, q, c, len(sums))
    var[:, n:] = 0
    return var


def preview(sums, c):
    """The RGB preview of the same accumulator: sum x 1.0f / float(samples)."""
    acc, _ = accumulate(sums)
    return acc * (F(1.0) / F(len(sums) * c))


# ---- the guided filter ------------------------------------------------------------------

def _lum(x):
    return (x[..., 0] + x[..., 1]) + x[..., 2]


def _smooth3(var):
    """g: dy outer, dx inner, a neighbour outside D contributes the centre's value."""
    n = var.shape[0]
    g = np.zeros_like(var)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            wt = W3[(dx == 0) + (dy == 0)]
            v = var.copy()
            px0, px1 = max(0, -dx), min(n, n - dx)
            py0, py1 = max(0, -dy), min(n, n - dy)
            if px0 < px1 and py0 < py1:
                v[py0:py1, px0:px1] = var[py0 + dy:py1 + dy, px0 + dx:px1 + dx]
            g = g + v * wt
    _f32(g)
    return g


def guided(frame, features, variance_plane, iterations, sigma_color, sigma_normal, sigma_albedo, sigma_depth,
           flags=0):
    """frame float32[H, W, 3], features float32[H, W, 8], variance_plane float32[H, W] ->
    (the filtered frame, the filtered variance).  iterations 0 selects the default; a sigma
    of 0 switches its term off."""
    frame = np.ascontiguousarray(frame)
    features = np.ascontiguousarray(features)
    variance_plane = np.ascontiguousarray(variance_plane)
    _f32(frame, features, variance_plane)
    height, width, _ = frame.shape
    assert features.shape == (height, width, 8) and variance_plane.shape == (height, width) and height <= width
    n = height
    iterations = iterations or R.DEFAULT_ITERATIONS
    assert 1 <= iterations <= 8
    one = F(1.0)
    sig = [F(s) for s in (sigma_color, sigma_normal, sigma_albedo, sigma_depth)]
    on = [bool(s > 0) for s in sig]
    _, inv_n, inv_a, inv_z = [one / s if o else F(0.0) for s, o in zip(sig, on)]
    col = frame[:, :n, :].copy()
    var = variance_plane[:, :n].copy()
    nrm = features[:, :n, 0:3]
    dep = features[:, :n, 3]
    alb = features[:, :n, 4:7]
    hit = np.ascontiguousarray(features[:, :n, 7]).view(np.uint32) != 0
    demod = bool(flags & DEMODULATE)
    with np.errstate(all="ignore"):
        if demod:
            big = hit[..., None] & (alb > A_MIN)
            col = np.where(big, col / alb, col).astype(F)
            am = ((alb[..., 0] + alb[..., 1]) + alb[..., 2]) * (one / F(3.0))
            vbig = hit & (am > A_MIN)
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
            lum = _lum(col)
            acc = np.zeros_like(col)
            wsum = np.zeros((n, n), F)
            vacc = np.zeros((n, n), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    px0, px1 = max(0, -s * dx), min(n, n - s * dx)
                    py0, py1 = max(0, -s * dy), min(n, n - s * dy)
                    if px0 >= px1 or py0 >= py1:
                        continue
                    P = (slice(py0, py1), slice(px0, px1))
                    Q = (slice(py0 + s * dy, py1 + s * dy), slice(px0 + s * dx, px1 + s * dx))
                    if dx == 0 and dy == 0:
                        w = R.H5[2] * R.H5[2]
                        acc[P] = acc[P] + col[Q] * w
                        wsum[P] = wsum[P] + w
                        vacc[P] = vacc[P] + var[Q] * (w * w)
                        continue
                    ok = hit[P] == hit[Q]
                    w = np.full(ok.shape, R.H5[dx + 2] * R.H5[dy + 2], F)
                    if on[0]:
                        t = one - np.abs(lum[P] - lum[Q]) * kl[P]
                        ok &= t > 0
                        w = w * t
                    if on[1]:
                        d = nrm[P] - nrm[Q]
                        t = one - ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) * inv_n
                        ok &= t > 0
                        w = w * t
                    if on[2]:
                        t = one - R._l1(alb[P] - alb[Q]) * inv_a
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
                    vacc[P] = np.where(ok, vacc[P] + var[Q] * (w * w), vacc[P])
            _f32(acc, wsum, vacc)
            col = acc / wsum[..., None]
            var = vacc / (wsum * wsum)
            _f32(col, var)
        if demod:
            col = np.where(big, col * alb, col).astype(F)
            var = np.where(vbig, var * (am * am), var).astype(F)
    out = frame.copy()
    out[:, :n, :] = col
    out_var = variance_plane.copy()
    out_var[:, :n] = var
    return out, out_var


def guided_dn(frame, features, variance_plane, dn, flags=0):
    """guided() with the fields of a zrt_denoise (_ffi.Denoise)."""
    return guided(frame, features, variance_plane, dn.iterations, dn.sigma_color, dn.sigma_normal, dn.sigma_albedo,
                  dn.sigma_depth, flags)

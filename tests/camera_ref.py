"""The camera-query reference (include/zrt.h "camera queries"), composed from oracle_render
alone, one sample at a time.  Test infrastructure: used by tests/test_camera_ref.py (CPU)
and tests/test_gpu_camera.py (GPU).

Sample s of pixel R = y * width + x:

  floats   r1, r2 = the first two floats of the stream of key(R, s) (O.prng_f32); a lens
           sample comes from the stream of key ^ LENS.
  model    restated here in numpy f32, nothing fused, in zrt.h's order, with the oracle's
           own sin, cos and sqrt (O.math1) for the transcendental steps: (o, tgt).
  colour   the 1 x 1, one-sample frame of radiance_ref.ray_camera(o, tgt) under
           radiance_ref.shifted_seed(seed, R, s): the oracle draws the same two jitter
           floats, its degenerate camera ignores them, and rayColor continues on the same
           stream.  (The degenerate camera turns a -0 target component into +0: targets
           must hold none, which sample_rays asserts - a condition on the test's cameras.)
  sums     radiance_ref.chunk_sums over the samples' colours; the mean is mean_of.
"""
import numpy as np

import radiance_ref as R
import zraytrace_amd as z

F = np.float32
LENS = 0xD1B54A32D192ED03
TWO_PI, PI = F(6.2831855), F(3.1415927)


def vec(v):
    return np.array([v.x, v.y, v.z], F)


def pixels_of(width, rect):
    """(x, y, R) of the rectangle's pixels, row-major from its bottom row."""
    x0, y0, w, h = rect
    ys, xs = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), indexing="ij")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    return xs, ys, ys.astype(np.int64) * width + xs


def plane_point(lens, u, v):
    """P(u, v) = (lower_left_corner + horizontal * u) + vertical * v (camera.zig:47-49)."""
    return ((vec(lens.lower_left_corner) + vec(lens.horizontal) * u) + vec(lens.vertical) * v).astype(F)


def lens_point(O, prng, key):
    """The thin lens' (a, b): pairs 2 f - 1 from the lens stream until a a + b b < 1."""
    f = O.prng_f32(prng, (key ^ LENS) & R.MASK64, 256)
    for k in range(0, 256, 2):
        a, b = F(2.0) * f[k] - F(1.0), F(2.0) * f[k + 1] - F(1.0)
        if a * a + b * b < F(1.0):
            return a, b
    raise AssertionError("128 lens samples in a row outside the disc")


def model(O, lens, u, v, prng, key):
    """(o, tgt) of one sample, in f32."""
    u, v = F(u), F(v)
    org = vec(lens.origin)
    au, av, aw = vec(lens.axis_u), vec(lens.axis_v), vec(lens.axis_w)
    if lens.kind == z.ZRT_LENS_PINHOLE:
        return org, plane_point(lens, u, v)
    if lens.kind == z.ZRT_LENS_THIN:
        a, b = lens_point(O, prng, key)
        return ((org + au * a) + av * b).astype(F), plane_point(lens, u, v)
    if lens.kind == z.ZRT_LENS_ORTHO:
        o = plane_point(lens, u, v)
        return o, (o + aw).astype(F)
    if lens.kind == z.ZRT_LENS_EQUIRECT:
        phi, theta = TWO_PI * u, PI * v
        sp, cp = O.math1("sin", [phi])[0], O.math1("cos", [phi])[0]
        st, ct = O.math1("sin", [theta])[0], O.math1("cos", [theta])[0]
        d = np.array([st * cp, -ct, st * sp], F)
        return org, (org + d).astype(F)
    assert lens.kind == z.ZRT_LENS_FISHEYE
    px, py = F(2.0) * u - F(1.0), F(2.0) * v - F(1.0)
    r = O.math1("sqrt", [px * px + py * py])[0]
    if r == 0:
        d = aw
    else:
        th = r * F(lens.half_fov)
        k = O.math1("sin", [th])[0] / r
        d = ((au * (px * k)) + av * (py * k)) + aw * O.math1("cos", [th])[0]
    assert d.dtype == F
    return org, (org + d).astype(F)


def sample_rays(O, lens, p, rect, first_sample, n_samples):
    """(R int64[n], o float32[n, k, 3], tgt float32[n, k, 3]) over the rectangle's n pixels and
    the k = n_samples samples from first_sample.  p: width, height, seed and prng are read."""
    xs, ys, Rs = pixels_of(p.width, rect)
    o = np.zeros((len(Rs), n_samples, 3), F)
    t = np.zeros((len(Rs), n_samples, 3), F)
    fw, fh = F(p.width), F(p.height)
    for i, (x, y, r) in enumerate(zip(xs, ys, Rs)):
        for j in range(n_samples):
            key = R.key_of(int(r), first_sample + j, p.seed)
            r1, r2 = O.prng_f32(p.prng, key, 2)
            u = ((F(x) + r1) - F(0.5)) / fw
            v = ((F(y) + r2) - F(0.5)) / fh
            assert u.dtype == F and v.dtype == F
            o[i, j], t[i, j] = model(O, lens, u, v, p.prng, key)
    assert not (np.signbit(t) & (t == 0)).any(), "a -0 target component"
    return Rs, o, t


def sample_colors(O, view, p, Rs, o, t, first_sample):
    """rayColor and the oracle's counters of every (pixel, sample): (float32[n, k, 3],
    uint64[n, COUNTERS]).  p: max_depth, bounded_volume_hierarchy, seed, prng are read."""
    n, k, _ = o.shape
    cols = np.zeros((n, k, 3), F)
    counters = np.zeros((n, len(R.COUNTERS)), np.uint64)
    for i in range(n):
        for j in range(k):
            q = R._params(p, 1, 1, 1, R.shifted_seed(p.seed, int(Rs[i]), first_sample + j))
            img, st = O.render(view, R.ray_camera(o[i, j], t[i, j]), q)
            cols[i, j] = img[0, 0]
            counters[i] += np.array([st[R._STATS[c]] for c in R.COUNTERS], np.uint64)
    return cols, counters


class Frame:
    """The reference of one call without ZRT_CQ_ACCUMULATE over samples [first_sample,
    first_sample + n_samples) of a rectangle (default: the frame): cols float32[n, k, 3],
    sum float32[n, 4], rgb float32[n, 3] and counters per pixel, pixels row-major over the
    rectangle from its bottom row.  prefix(k) is the reference of the first k samples."""

    def __init__(self, O, view, p, lens, n_samples, rect=None, first_sample=0, _from=None):
        self.p, self.rect = p, rect or (0, 0, p.width, p.height)
        if _from is None:
            self.R, self.o, self.t = sample_rays(O, lens, p, self.rect, first_sample, n_samples)
            self.cols, self.per_sample = self._colors(O, view, first_sample)
        else:
            self.R, self.o, self.t = _from.R, _from.o[:, :n_samples], _from.t[:, :n_samples]
            self.cols, self.per_sample = _from.cols[:, :n_samples], _from.per_sample[:, :n_samples]
        self.counters = self.per_sample.sum(1, dtype=np.uint64)
        self.sum = R.chunk_sums(self.cols, p.sample_chunk)
        self.rgb = R.mean_of(self.sum, n_samples)
        self.info = R.info_of(self.counters)

    def _colors(self, O, view, first_sample):
        n, k, _ = self.o.shape
        cols = np.zeros((n, k, 3), F)
        per = np.zeros((n, k, len(R.COUNTERS)), np.uint64)
        for j in range(k):
            c, cnt = sample_colors(O, view, self.p, self.R, self.o[:, j:j + 1], self.t[:, j:j + 1], first_sample + j)
            cols[:, j], per[:, j] = c[:, 0], cnt
        return cols, per

    def prefix(self, n_samples):
        return Frame(None, None, self.p, None, n_samples, self.rect, _from=self)

    def image(self, a):
        """Per-pixel values as [h, w, ...] of the rectangle."""
        a = np.asarray(a)
        return a.reshape((self.rect[3], self.rect[2]) + a.shape[1:])


def lens_of_camera(cam, kind=z.ZRT_LENS_PINHOLE):
    """The lens whose plane is a zrt_camera's (axes zero, so a thin lens of aperture 0)."""
    return z._ffi.Lens(kind=kind, origin=cam.origin, lower_left_corner=cam.lower_left_corner,
                       horizontal=cam.horizontal, vertical=cam.vertical, half_fov=1.0)


def lens_init_np(O, kind, look_from, look_at, vup, vfov, aspect, aperture, focus_dist, fisheye_fov):
    """zrt_lens_init restated in numpy f32 on Camera.init's u, v, w and h (camera.zig:17-35):
    a dict of the descriptor's fields.  tan as numpy's f32 (the host's tanf)."""
    def unit(a):
        return (a / np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])).astype(F)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)

    lf, la, up = (np.asarray(a, F) for a in (look_from, look_at, vup))
    theta = F(np.pi) * F(vfov) / F(180.0)
    h = np.tan(theta / F(2.0))
    assert h.dtype == F
    vh = F(2.0) * h
    vw = F(aspect) * vh
    w = unit(lf - la)
    u = unit(cross(up, w))
    v = cross(w, u)
    fd = F(focus_dist)
    hor, ver = u * (fd * vw), v * (fd * vh)
    frame = kind in (z.ZRT_LENS_ORTHO, z.ZRT_LENS_FISHEYE)
    half = F(aperture) * F(0.5)
    return {"origin": lf, "horizontal": hor, "vertical": ver,
            "lower_left_corner": ((lf - hor * F(0.5)) - ver * F(0.5)) - w * fd,
            "axis_u": u if frame else u * half, "axis_v": v if frame else v * half, "axis_w": -w,
            "half_fov": F(fisheye_fov) * (F(np.pi) / F(360.0))}


def lens_from_camera_np(kind, cam, aperture, focus_dist, fisheye_fov):
    """zrt_lens_from_camera restated in numpy f32, in zrt.h's order: a dict of the descriptor's fields."""
    def length(a):
        return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])

    org, llc, hor, ver = vec(cam.origin), vec(cam.lower_left_corner), vec(cam.horizontal), vec(cam.vertical)
    axis = ((llc + hor * F(0.5)) + ver * F(0.5)) - org
    dist = length(axis)
    assert dist.dtype == F
    fwd, u, v = axis * (F(1.0) / dist), hor * (F(1.0) / length(hor)), ver * (F(1.0) / length(ver))
    out = {"origin": org, "lower_left_corner": llc, "horizontal": hor, "vertical": ver}
    if focus_dist > 0:
        fd = F(focus_dist)
        s = fd / dist
        h2, v2 = hor * s, ver * s
        out.update(horizontal=h2, vertical=v2, lower_left_corner=((org - h2 * F(0.5)) - v2 * F(0.5)) + fwd * fd)
    frame = kind in (z.ZRT_LENS_ORTHO, z.ZRT_LENS_FISHEYE)
    half = F(aperture) * F(0.5)
    out.update(axis_u=u if frame else u * half, axis_v=v if frame else v * half, axis_w=fwd,
               half_fov=F(fisheye_fov) * (F(np.pi) / F(360.0)))
    assert all(np.asarray(a).dtype == F for a in out.values())
    return out

"""The ambient-occlusion reference (include/zrt.h "ambient occlusion"), composed on the CPU
from pieces that are pinned elsewhere.  Test infrastructure: used by tests/test_ao_ref.py
(CPU) and tests/test_gpu_ao.py (GPU).

  features      denoise_ref.expected_features: the first hits, from the oracle;
  the origin    denoise_ref.pixel_rays / unit: P = o + dir * t per component in f32;
  the direction N + randomUnitVector, the latter O.sample_vector(prng, key, 3) on the
                counter mode's key of (pixel, sample) - the RAW sum: the hooks normalise;
  occluded      anyhit_ref.leafwise under the BVH, literal_list without one, at t_max =
                the radius.

The occlusion of (pixel, sample s) does not depend on how many samples a call takes, so
an AoCase keeps it per sample index and serves every (first_sample, n_samples) from it.
"""
import numpy as np

import anyhit_ref as A
import denoise_ref as R

F = np.float32
POISON = 0xFFFFFFFF
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def key_of(x, y, width, s, seed):
    """The counter mode's key (oracle.h): ((y * width + x) << 16 | s) + seed * 0x9E3779B97F4A7C15."""
    return ((((y * width + x) << 16) | s) + seed * GOLDEN) & MASK64


def classify(features):
    """Per pixel of D (the first `height` columns): miss, poisoned, hit (bool[h, n] each)."""
    h = features.shape[0]
    f = np.ascontiguousarray(features[:, :h])
    miss = np.ascontiguousarray(f[..., 7]).view(np.uint32) == 0
    poison = ~miss & np.isnan(f[..., 0:4]).any(-1)
    return miss, poison, ~miss & ~poison


class AoCase:
    """One scene, camera, frame size, feature buffer, radius, seed and PRNG."""

    def __init__(self, O, view, camera, width, height, radius=np.inf, seed=42, prng=0, bvh=True, features=None):
        self.O, self.view, self.camera = O, view, camera
        self.width, self.height, self.radius, self.seed, self.prng = width, height, F(radius), seed, prng
        self.scene = A.scene_struct(view)
        self.use_bvh = bool(bvh) and self.scene.n_prims > 10
        if features is None:
            features, _ = R.expected_features(O, view, camera, width, height, bvh=bvh)
        self.features = np.ascontiguousarray(features, F)
        self.miss, self.poison, self.hit = classify(self.features)
        self.ys, self.xs = np.nonzero(self.hit)
        o, d = R.pixel_rays(camera, width, height)
        du = R.unit(d)
        t = self.features[..., 3]
        loc = o + du * t[..., None]  # ray.zig:14-16, per component
        assert loc.dtype == F
        self.P = loc[self.ys, self.xs]
        self.N = self.features[self.ys, self.xs, 0:3]
        self.nodes = O.bvh_build(view)[:4] if self.use_bvh else None
        self._occ = {}  # sample index -> bool[hit pixels]
        self._dir = {}

    def directions(self, s):
        """N + randomUnitVector of sample s for every hit pixel (raw, float32[k, 3])."""
        if s not in self._dir:
            r = np.array([self.O.sample_vector(self.prng, key_of(int(x), int(y), self.width, s, self.seed), 3)
                          for y, x in zip(self.ys, self.xs)], F).reshape(-1, 3)
            self._dir[s] = self.N + r
            assert self._dir[s].dtype == F
        return self._dir[s]

    def _need(self, samples):
        todo = [s for s in samples if s not in self._occ]
        if not todo or len(self.ys) == 0:
            for s in todo:
                self._occ[s] = np.zeros(0, bool)
            return
        k = len(self.ys)
        o = np.concatenate([self.P] * len(todo))
        d = np.concatenate([self.directions(s) for s in todo])
        tm = np.full(len(o), self.radius, F)
        if self.use_bvh:
            occ = A.leafwise(self.O, self.view, self.nodes, o, d, tm)
        else:
            occ = A.literal_list(self.O, self.view, o, d, tm)
        for j, s in enumerate(todo):
            self._occ[s] = occ[j * k:(j + 1) * k]

    def occluded(self, first_sample, n_samples):
        """bool[hit pixels, n_samples] of samples first_sample .. first_sample + n_samples - 1."""
        samples = range(first_sample, first_sample + n_samples)
        self._need(samples)
        return np.stack([self._occ[s] for s in samples], 1) if len(self.ys) else np.zeros((0, n_samples), bool)

    def counts(self, first_sample, n_samples):
        """c per pixel of the whole frame for one call without ZRT_AO_ACCUMULATE (uint32[h, w];
        POISON on a poisoned pixel, 0 outside D)."""
        c = np.zeros((self.height, self.width), np.uint32)
        n = self.height
        d = c[:, :n]
        d[self.miss] = n_samples
        d[self.poison] = POISON
        d[self.ys, self.xs] = (~self.occluded(first_sample, n_samples)).sum(1)
        return c

    def expected(self, first_sample, n_samples, prior=None):
        """(clear uint32[h, w], ao float32[h, w]) of one call; prior: the plane a call with
        ZRT_AO_ACCUMULATE starts from (None: a call without the flag)."""
        c = self.counts(first_sample, n_samples)
        n = self.height
        inside = np.zeros(c.shape, bool)
        inside[:, :n] = True
        bad = c == POISON
        if prior is None:
            clear, den = c, F(n_samples)
        else:
            prior = np.asarray(prior, np.uint32)
            bad = bad | (prior == POISON)
            clear, den = (prior + c).astype(np.uint32), F(first_sample + n_samples)
        clear = np.where(inside, np.where(bad, np.uint32(POISON), clear), 0).astype(np.uint32)
        with np.errstate(all="ignore"):
            ao = clear.astype(F) / den
        ao = np.where(bad & inside, F(np.nan), ao).astype(F)
        return clear, ao

    def rays(self, first_sample, n_samples):
        """The AO rays of a call, pixel-major: (origins[k n, 3], raw directions[k n, 3])."""
        d = np.stack([self.directions(s) for s in range(first_sample, first_sample + n_samples)], 1)
        return np.repeat(self.P, n_samples, 0), d.reshape(-1, 3)

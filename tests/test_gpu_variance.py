"""The variance plane of an accumulation run against the oracle, bit for bit.

The oracle delivers a frame's individual chunk sums (tests/denoise_guided_ref.chunk_sums:
a render of one chunk with the seed moved to that chunk's streams); adding them in order
in numpy gives the accumulator's sums and second moment, and the f32 expressions of
include/zrt.h "the variance plane" give the plane zrt_ctx_accum_variance must write -
for a plain run however it was split into passes, and for an adaptive run with every
tile's own chunk count.  The RGB previews of the same runs stay the oracle's frames.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O

import denoise_guided_ref as G
import test_gpu_adaptive as A
import test_gpu_loop_edges as E
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = z._ffi.ZRT_E_INVALID, z._ffi.ZRT_E_UNSUPPORTED
F = np.float32
DEPTH = 8

_SUMS = {}  # (scene, width, height, chunk, depth, prng, seed) -> the chunk sums computed so far


def chunk_of(p):
    return p.sample_chunk or 32


def sums_of(scenes, which, p, k):
    """The first k chunk sums of p's frame, from the oracle, computed once and shared."""
    c = chunk_of(p)
    key = (which, p.width, p.height, c, p.max_depth, p.prng, p.seed)
    have = _SUMS.get(key)
    if have is None or len(have) < k:
        _, view, cam = E.scene_of(scenes, which)
        have = G.chunk_sums(O, view, cam, dataclasses.replace(p, sample_chunk=c), k)
        have.setflags(write=False)
        _SUMS[key] = have
    return have[:k]


def params(w=24, h=24, spp=32, chunk=4, prng=z.ZRT_PRNG_XOROSHIRO128, **kw):
    return z.RenderParams(w, h, spp, DEPTH, prng=prng, sample_chunk=chunk, **kw)


def assert_plane(got, want, what):
    g, w = got.view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)
    same = (g == w) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        i = tuple(np.argwhere(~same)[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {g.size} values differ, first at {i}: "
                             f"got {got[i]!r} want {want[i]!r}")


class Run:
    """A context with its tile, plane and frame buffers."""

    def __init__(self, scenes, which, p):
        import torch
        self.keep, self.view, self.cam = E.scene_of(scenes, which)
        self.p = p
        self.ctx = z.RenderContext(self.view, p)
        n = self.ctx.tile_count(p)
        self.tiles = torch.zeros(n * 64 * 3, dtype=torch.float32, device="cuda")
        self.var_tiles = torch.full((max(1, n) * 64,), -7.0, dtype=torch.float32, device="cuda")
        self.dev_frame = torch.zeros(p.height * p.width * 3, dtype=torch.float32, device="cuda")
        self.dev_plane = torch.full((p.height * p.width,), -7.0, dtype=torch.float32, device="cuda")

    def frame(self):
        import torch
        self.ctx.assemble(self.p, self.tiles.data_ptr(), self.dev_frame.data_ptr())
        torch.cuda.synchronize()
        return self.dev_frame.cpu().numpy().reshape(self.p.height, self.p.width, 3)

    def variance(self):
        """zrt_ctx_accum_variance, assembled (one rank) into the frame's layout."""
        import torch
        self.ctx.accum_variance(self.var_tiles.data_ptr())
        self.ctx.assemble_plane(self.p, self.var_tiles.data_ptr(), self.dev_plane.data_ptr())
        torch.cuda.synchronize()
        return self.dev_plane.cpu().numpy().reshape(self.p.height, self.p.width)

    def close(self):
        self.ctx.close()


def check_plain(scenes, which, p, passes):
    """A plain run in `passes`: after every pass that leaves two or more chunks the plane is
    the oracle-derived one, and the preview is the oracle's frame at that many samples."""
    c = chunk_of(p)
    run = Run(scenes, which, p)
    try:
        run.ctx.accum_begin(run.cam, p)
        done = 0
        for n in passes:
            run.ctx.accum_pass(n, run.tiles.data_ptr())
            done += n
            img = run.frame()
            ref = E.oracle_frame(scenes, which, dataclasses.replace(p, samples_per_pixel=done))[0]
            P.assert_bit_exact(img, ref)
            if done // c < 2:
                continue
            s = sums_of(scenes, which, p, done // c)
            assert (G.preview(s, c).view(np.uint32) == ref.view(np.uint32)).all()  # (the chunk sums are the frame's)
            want = G.frame_variance(s, c, p.height)
            got = run.variance()
            assert_plane(got, want, f"{which} {p.width}x{p.height} after {done} samples")
        assert (want[:, :p.height] > 0).any() and np.isfinite(want).all()
        return got
    finally:
        run.close()


# ---- plain runs -------------------------------------------------------------------------

PASSES = {"one-pass": (32,), "2+6-chunks": (8, 24), "8-passes": (4,) * 8}


@pytest.mark.parametrize("split", list(PASSES))
@pytest.mark.parametrize("name", ["bubbles", "glass-inside"])
def test_variance_however_the_run_is_split(scenes, name, split):
    """24 x 24, chunk 4, 32 spp as one pass of 8 chunks, 2 then 6 chunks, and 8 passes of one."""
    check_plain(scenes, name, params(), PASSES[split])


@pytest.mark.parametrize("name", ["bubbles", "glass-inside"])
def test_variance_xoshiro(scenes, name):
    check_plain(scenes, name, params(prng=z.ZRT_PRNG_XOSHIRO256), (8, 24))


def test_variance_of_two_chunks(scenes):
    """k = 2 (8 spp): the smallest case, sc = 1 / (1 x 16)."""
    check_plain(scenes, "bubbles", params(spp=8), (8,))


def test_variance_default_chunk(scenes):
    """sample_chunk 0 selects 32: 64 spp are two chunks."""
    check_plain(scenes, "glass-inside", params(spp=64, chunk=0), (64,))


def test_variance_wide_frame(scenes):
    """40 x 24: the columns outside the rendered square are zero."""
    got = check_plain(scenes, "bubbles", params(w=40), (32,))
    assert not got[:, 24:].any() and got[:, :24].any()


@pytest.mark.parametrize("stride", [0, 4], ids=["packed", "padded"])
def test_variance_of_three_ranks(scenes, stride):
    """world_size 3 on one GPU: every rank writes its own tiles' plane (rank 1 among them), and
    zrt_ctx_assemble_plane puts the gathered planes into the frame's layout."""
    import torch
    p = params()
    want = G.frame_variance(sums_of(scenes, "bubbles", p, 8), 4, 24)
    counts = [3, 3, 3]  # 9 tiles dealt round-robin
    per = stride or 3
    gathered = torch.full((3 * per * 64,), -7.0, dtype=torch.float32, device="cuda")
    runs = []
    try:
        for rank in range(3):
            pr = dataclasses.replace(p, rank=rank, world_size=3)
            run = Run(scenes, "bubbles", pr)
            runs.append(run)
            assert run.ctx.tile_count(pr) == counts[rank]
            run.ctx.accum_begin(run.cam, pr)
            run.ctx.accum_pass(32, run.tiles.data_ptr())
            run.ctx.accum_variance(run.var_tiles.data_ptr())
            torch.cuda.synchronize()
            gathered[rank * per * 64:rank * per * 64 + counts[rank] * 64] = run.var_tiles[:counts[rank] * 64]
        plane = torch.full((24 * 24,), -7.0, dtype=torch.float32, device="cuda")
        runs[1].ctx.assemble_plane(runs[1].p, gathered.data_ptr(), plane.data_ptr(), stride_tiles=stride)
        torch.cuda.synchronize()
        assert_plane(plane.cpu().numpy().reshape(24, 24), want, f"3 ranks, stride {stride}")
        # rank 1's own tiles: tile t = 3 lt + 1
        tiles = runs[1].var_tiles.cpu().numpy().reshape(-1, 8, 8)
        for lt, t in enumerate((1, 4, 7)):
            ty, tx = divmod(t, 3)
            assert_plane(tiles[lt], want[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8], f"rank 1 tile {t}")
    finally:
        for run in runs:
            run.close()


# ---- an adaptive run ----------------------------------------------------------------------

def test_variance_of_an_adaptive_run(scenes):
    """32 x 32, chunk 4, first level 8, cap 64 (levels 8, 16, 32, 64): the tolerance whose
    oracle-derived decisions freeze tiles at the most distinct levels - two at least - and
    every tile's variance from its own k = samples / 4 chunk sums."""
    p = params(w=32, h=32, spp=64)
    ex = A.expected_run(scenes, "bubbles", p, 8)
    assert ex.levels == [8, 16, 32, 64]
    final = ex.samples(len(ex.steps) - 1)
    assert len(set(final.tolist())) >= 2, (ex.tol, final)
    sums = sums_of(scenes, "bubbles", p, 16)
    want = np.zeros((32, 32), F)
    planes = {int(n): G.frame_variance(sums[:int(n) // 4], 4, 32) for n in set(final.tolist())}
    for t, (x0, x1, y0, y1) in enumerate(A.tile_boxes(p)):
        want[y0:y1, x0:x1] = planes[int(final[t])][y0:y1, x0:x1]
    run = Run(scenes, "bubbles", p)
    try:
        run.ctx.adapt_begin(run.cam, p, ex.tol, 8)
        for _ in ex.steps:
            run.ctx.adapt_level(run.tiles.data_ptr())
        np.testing.assert_array_equal(run.ctx.adapt_samples(), final)
        P.assert_bit_exact(run.frame(), ex.frames[-1])
        got = run.variance()
        assert_plane(got, want, f"adaptive, tolerance {ex.tol}")
        # a uniform plane of any single k differs: the tiles' own counts were used
        for n, plane in planes.items():
            assert (got.view(np.uint32) != plane.view(np.uint32)).any(), n
    finally:
        run.close()


# ---- refusals ---------------------------------------------------------------------------

def test_variance_refusals(scenes):
    """No live run, no pass yet, fewer than two chunks, and after a ragged pass: ZRT_E_INVALID;
    a new run on the same context is served again."""
    p = params(spp=10)
    run = Run(scenes, "bubbles", p)
    try:
        def refused(word):
            with pytest.raises(z.ZrtError) as e:
                run.ctx.accum_variance(run.var_tiles.data_ptr())
            assert e.value.code == E_INVALID and word in str(e.value), str(e.value)

        refused("no run is live")
        run.ctx.accum_begin(run.cam, p)
        refused("no pass")
        run.ctx.accum_pass(4, run.tiles.data_ptr())
        refused("fewer than two chunks")
        run.ctx.accum_pass(6, run.tiles.data_ptr())  # 4 + 2: the run's ragged last pass
        P.assert_bit_exact(run.frame(), E.oracle_frame(scenes, "bubbles", p)[0])
        refused("not whole chunks")
        run.ctx.render_tiles(run.cam, p, run.tiles.data_ptr())  # a plain render ends the run
        run.ctx.sync()
        refused("no run is live")
        run.ctx.accum_begin(run.cam, p)
        run.ctx.accum_pass(8, run.tiles.data_ptr())
        want = G.frame_variance(sums_of(scenes, "bubbles", p, 2), 4, 24)
        assert_plane(run.variance(), want, "a new run after the refusals")
    finally:
        run.close()


def test_variance_after_a_device_error(scenes, monkeypatch):
    """test_gpu_progressive's safe hook (the STATS flavour told its row buffers hold nothing: the
    device check skips the access and raises the error flag): the plane is NaN and the status is
    the run's sticky ZRT_E_UNSUPPORTED; a new run without the cap gives a finite plane."""
    import torch
    p = z.RenderParams(128, 128, 4, 20, flags=z.ZRT_FLAG_STATS, sample_chunk=2)
    monkeypatch.setenv("ZRT_POOL", "0")
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS", "2")
    run = Run(scenes, 3, p)
    try:
        monkeypatch.setenv("ZRT_DEBUG_ROW_CAP", "0")
        run.ctx.accum_begin(run.cam, p)
        run.ctx.accum_pass(4, run.tiles.data_ptr())
        with pytest.raises(z.ZrtError, match="past its buffer") as e:
            run.ctx.accum_variance(run.var_tiles.data_ptr())
        assert e.value.code == E_UNSUPPORTED
        torch.cuda.synchronize()
        assert np.isnan(run.var_tiles.cpu().numpy()).all()
        monkeypatch.delenv("ZRT_DEBUG_ROW_CAP")
        run.ctx.accum_begin(run.cam, p)
        run.ctx.accum_pass(4, run.tiles.data_ptr())
        got = run.variance()
        assert np.isfinite(got).all() and (got >= 0).all() and (got > 0).any()
    finally:
        run.close()

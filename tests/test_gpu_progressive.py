"""Progressive rendering: sample passes accumulated into a resident frame.

A sample's stream is keyed by (pixel, sample, seed) and a pixel is the sequential
sum of its chunk sums times 1 / spp, so after any prefix of whole chunks the
accumulated frame, scaled by 1 / done, is the oracle's full render at
samples_per_pixel = done - bit for bit, with its Progress counters and scanline
rows (zrt_ctx_accum_begin / _pass / _info, zrt_render_progressive, the CLI's
ZRT_PASS_SAMPLES).  Every prefix below is compared with the existing oracle
through test_gpu_loop_edges's shared frames.

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O  # noqa: F401  (the oracle behind E.oracle_frame)

import test_gpu_loop_edges as E
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = z._ffi.ZRT_E_INVALID, z._ffi.ZRT_E_UNSUPPORTED
SCANLINES = z.ZRT_FLAG_SCANLINES


def png_quantize(img):
    """tests/test_image_io.py's: u8(std.math.clamp(255.999 * c, 0, 255)) in f32, math.min / max
    as `x < y ? x : y` (rows not flipped: only equality per pixel is used here)."""
    v = (np.float32(255.999) * img.astype(np.float32)).astype(np.float32)
    m = np.where(v < 255, v, np.float32(255))
    c = np.where(np.float32(0) > m, np.float32(0), m)
    return np.trunc(c).astype(np.uint8)


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


class Run:
    """A context with its tile and frame buffers; frame() assembles and reads back."""

    def __init__(self, scenes, which, p):
        import torch
        self.keep, self.view, self.cam = E.scene_of(scenes, which)
        self.p = p
        self.ctx = z.RenderContext(self.view, p)
        self.tiles = torch.zeros(self.ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
        self.dev_frame = torch.zeros(p.height * p.width * 3, dtype=torch.float32, device="cuda")

    def begin(self, p=None):
        self.p = p or self.p
        self.ctx.accum_begin(self.cam, self.p)

    def step(self, n):
        """One pass; the assembled frame (no status check: the caller syncs)."""
        import torch
        self.ctx.accum_pass(n, self.tiles.data_ptr())
        self.ctx.assemble(self.p, self.tiles.data_ptr(), self.dev_frame.data_ptr())
        torch.cuda.synchronize()
        return self.dev_frame.cpu().numpy().reshape(self.p.height, self.p.width, 3)

    def close(self):
        self.ctx.close()


def check_metrics(info, new, prev, n, done):
    """zrt_pass_info against the frames: the pixels whose 8-bit PNG value changed, and the
    largest |new - prev| in f32 by bits (a NaN difference is skipped, as the kernel skips it)."""
    assert (info["samples_done"], info["pass_samples"]) == (done, n)
    assert info["changed_pixels"] == int((png_quantize(new) != png_quantize(prev)).any(axis=2).sum())
    d = np.abs(new.astype(np.float32) - prev.astype(np.float32))
    d = d[~np.isnan(d)]
    want = d.max() if d.size else np.float32(0)
    assert f32_bits(info["max_abs_change"]) == f32_bits(want), (info["max_abs_change"], want)


def check_prefixes(scenes, which, p, passes, metrics=True):
    """Every prefix of `passes` against the oracle at spp = done: frame, Progress counters,
    scanline rows (when flagged), pass metrics.  Returns (last frame, last stats, infos)."""
    run = Run(scenes, which, p)
    try:
        run.begin()
        done, prev, infos = 0, np.zeros((p.height, p.width, 3), np.float32), []
        for n in passes:
            img = run.step(n)
            done += n
            q = dataclasses.replace(p, samples_per_pixel=done)
            ref, rs, rrows = E.oracle_frame(scenes, which, q)
            P.assert_bit_exact(img, ref)
            st = run.ctx.stats()
            for k in P.COUNTERS:
                assert st[k] == rs[k], (k, done)
            if p.flags & SCANLINES:
                np.testing.assert_array_equal(run.ctx.scanlines(p.height), rrows)
            info = run.ctx.accum_info()
            print(f"{which} done {done}: {info}")
            if metrics:
                check_metrics(info, ref, prev, n, done)
            infos.append(info)
            prev = ref
        return img, st, infos
    finally:
        run.close()


# ---- 1. every prefix, every loop ------------------------------------------------------

PASSES = (3, 6, 3)


def prefix_params(loop, prng, monkeypatch, flags=SCANLINES):
    p = E.frame_params(12, E.PRNGS[prng], spp=12, chunk=3)
    p = dataclasses.replace(p, bounded_volume_hierarchy=loop not in E.LIST_LOOPS)
    p = E.set_edge_loop(monkeypatch, loop, p)
    return dataclasses.replace(p, flags=p.flags | flags)


@pytest.mark.parametrize("prng", list(E.PRNGS))
@pytest.mark.parametrize("loop", E.BVH_LOOPS + E.LIST_LOOPS)
@pytest.mark.parametrize("name", ["glass-inside", "wraps"])
def test_every_prefix_every_loop(scenes, name, loop, prng, monkeypatch):
    """24 x 24, depth 12, chunk 3, cap 12 in passes of 3 / 6 / 3 with the scanline rows:
    after each pass the frame, counters and rows are the oracle's at spp = done; the forced
    loop ran; the last prefix is also z.render's frame at spp 12."""
    p = prefix_params(loop, prng, monkeypatch)
    img, st, infos = check_prefixes(scenes, name, p, PASSES)
    assert st["sampling_loop"] == E.LOOPS[loop][3]
    assert [i["schedule_ms"] for i in infos] == [0.0, 0.0, 0.0]  # (cap < 128: no probe)
    assert st["render_ms"] >= sum(i["render_ms"] for i in infos) * 0.999 > 0
    _, view, cam = E.scene_of(scenes, name)
    full, fs = z.render(view, cam, p)
    assert P.same_bits(img, full).all()
    for k in P.COUNTERS:
        assert fs[k] == st[k], k


@pytest.mark.parametrize("name", ["glass-inside", "wraps"])
def test_every_prefix_stats_flavour(scenes, name, monkeypatch):
    """The STATS flavour of the lockstep loop accumulates the same bits (and counts
    rays_processed itself over the passes)."""
    p = prefix_params("lockstep", "xoroshiro", monkeypatch, flags=SCANLINES | z.ZRT_FLAG_STATS)
    img, st, _ = check_prefixes(scenes, name, p, PASSES)
    assert st["sampling_loop"] == 3 and st["node_visits"] > 0


# ---- 2. ragged ends -------------------------------------------------------------------

def test_ragged_ends(scenes):
    """20 x 13 (pixels with x >= height stay 0), chunk 3, passes 6 then 4 of a cap of 12:
    both prefixes are the oracle's, the ragged pass ends the run's growth, and a new begin
    starts from a clean accumulator."""
    p = dataclasses.replace(E.frame_params(8, w=20, h=13, spp=12, chunk=3), flags=SCANLINES)
    run = Run(scenes, 4, p)
    try:
        run.begin()
        for n, done in ((6, 6), (4, 10)):
            img = run.step(n)
            run.ctx.sync()
            ref, rs, rrows = E.oracle_frame(scenes, 4, dataclasses.replace(p, samples_per_pixel=done))
            P.assert_bit_exact(img, ref)
            assert not img[:, 13:].any() and img[:, :13].any()
            st = run.ctx.stats()
            for k in P.COUNTERS:
                assert st[k] == rs[k], (k, done)
            np.testing.assert_array_equal(run.ctx.scanlines(13), rrows)
        with pytest.raises(z.ZrtError) as e:
            run.step(2)
        assert e.value.code == E_INVALID and "chunk boundary" in str(e.value)
        # no residue: a new run's first pass is the frame of its own size
        run.begin()
        img = run.step(6)
        ref, rs, _ = E.oracle_frame(scenes, 4, dataclasses.replace(p, samples_per_pixel=6))
        P.assert_bit_exact(img, ref)
        assert run.ctx.stats()["reflections"] == rs["reflections"]
        info = run.ctx.accum_info()
        check_metrics(info, ref, np.zeros_like(ref), 6, 6)
    finally:
        run.close()


def test_tall_frame_is_refused(scenes):
    """13 x 20: height > width is refused by a run as by every render (the reference would
    write past the image, raytrace.zig:168)."""
    s = scenes(4)
    ctx = z.RenderContext(s, E.frame_params(8, w=20, h=13, spp=12, chunk=3))
    try:
        with pytest.raises(z.ZrtError) as e:
            ctx.accum_begin(s.camera, E.frame_params(8, w=13, h=20, spp=12, chunk=3))
        assert e.value.code == E_INVALID and "height > width" in str(e.value)
    finally:
        ctx.close()


# ---- 3. the top of the sample range ----------------------------------------------------

@pytest.mark.parametrize("which,bvh", [(1, False), ("glass-inside", True)], ids=["list", "bvh"])
def test_top_of_sample_range(scenes, which, bvh):
    """2 x 2, depth 3, chunk 4096, cap 65535 in passes of 61440 and 4095: the second pass's
    keys are shifted by 61440 and reach sample 65534; one more sample is refused."""
    p = z.RenderParams(2, 2, 65535, 3, sample_chunk=4096, bounded_volume_hierarchy=bvh)
    run = Run(scenes, which, p)
    try:
        run.begin()
        for n, done in ((61440, 61440), (4095, 65535)):
            img = run.step(n)
            ref, rs, _ = E.oracle_frame(scenes, which, dataclasses.replace(p, samples_per_pixel=done))
            P.assert_bit_exact(img, ref)
            st = run.ctx.stats()
            for k in P.COUNTERS:
                assert st[k] == rs[k], (k, done)
        with pytest.raises(z.ZrtError) as e:
            run.step(1)
        assert e.value.code == E_INVALID
    finally:
        run.close()


# ---- 4. behind the probe ---------------------------------------------------------------

def test_behind_the_probe(scenes, monkeypatch):
    """16 x 16, chunk 32, cap 256 in passes of 64, the default FAST loop: the run schedules
    once (pass 1 probes, passes 2-4 reuse its order), every prefix is the oracle's; with a
    cap of 64 no pass schedules."""
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES"):
        monkeypatch.delenv(k, raising=False)
    p = E.frame_params(12, w=16, h=16, spp=256, chunk=0)
    run = Run(scenes, "wraps", p)
    try:
        run.begin()
        orders = []
        for i in range(4):
            img = run.step(64)
            done = 64 * (i + 1)
            ref, rs, _ = E.oracle_frame(scenes, "wraps", dataclasses.replace(p, samples_per_pixel=done))
            P.assert_bit_exact(img, ref)
            info = run.ctx.accum_info()
            assert (info["schedule_ms"] > 0) == (i == 0), info
            orders.append(run.ctx.debug_schedule()[1])
            st = run.ctx.stats()
            for k in P.COUNTERS:
                assert st[k] == rs[k], (k, done)
        assert len(orders[0]) == 4 and sorted(orders[0]) == [0, 1, 2, 3]
        for o in orders[1:]:
            np.testing.assert_array_equal(o, orders[0])
        assert st["schedule_ms"] > 0 and st["render_ms"] > st["schedule_ms"]
        # cap 64: below the rule's 128 samples
        run.begin(dataclasses.replace(p, samples_per_pixel=64))
        img = run.step(64)
        P.assert_bit_exact(img, E.oracle_frame(scenes, "wraps", dataclasses.replace(p, samples_per_pixel=64))[0])
        assert run.ctx.accum_info()["schedule_ms"] == 0 and len(run.ctx.debug_schedule()[1]) == 0
    finally:
        run.close()


# ---- 5. metrics ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["glass-inside", "wraps"])
def test_pass_metrics(scenes, name, monkeypatch):
    """Case 1's lockstep run: per pass, changed_pixels is the count from png_quantize of the
    oracle's consecutive prefix frames (zeros before pass 1) and max_abs_change is
    np.abs(new - prev).max() in f32, by bits (check_metrics, inside check_prefixes)."""
    p = prefix_params("lockstep", "xoroshiro", monkeypatch)
    _, _, infos = check_prefixes(scenes, name, p, PASSES, metrics=True)
    assert infos[0]["changed_pixels"] > 0 and infos[0]["max_abs_change"] > 0
    assert infos[0]["changed_pixels"] <= 24 * 24


# ---- 6. run life cycle -----------------------------------------------------------------

def test_run_life_cycle(scenes):
    p = E.frame_params(8, spp=12, chunk=3)
    run = Run(scenes, 4, p)
    try:
        with pytest.raises(z.ZrtError) as e:  # before any begin
            run.step(3)
        assert e.value.code == E_INVALID
        run.begin()
        run.step(3)
        with pytest.raises(z.ZrtError) as e:
            run.step(0)
        assert e.value.code == E_INVALID
        with pytest.raises(z.ZrtError) as e:
            run.step(12)
        assert e.value.code == E_INVALID
        # a plain render between passes ends the run
        run.ctx.render_tiles(run.cam, p, run.tiles.data_ptr())
        run.ctx.sync()
        with pytest.raises(z.ZrtError) as e:
            run.step(3)
        assert e.value.code == E_INVALID and "no accumulation run" in str(e.value)
        with pytest.raises(z.ZrtError):
            run.ctx.accum_info()
        run.begin()
        img = run.step(3)
        P.assert_bit_exact(img, E.oracle_frame(scenes, 4, dataclasses.replace(p, samples_per_pixel=3))[0])
    finally:
        run.close()


def test_sticky_device_error(scenes, monkeypatch):
    """test_device_row_bounds_check_reports's safe hook (scene 3, 128 x 128, 4 spp, depth 20,
    the STATS flavour told its row buffers hold nothing: the device check skips the access
    and raises the error flag): the erroring pass gives an all-NaN frame and the error, the
    next pass is refused, and a new run without the cap is exact again."""
    s = scenes(3)
    p = z.RenderParams(128, 128, 4, 20, flags=z.ZRT_FLAG_STATS, sample_chunk=2)
    monkeypatch.setenv("ZRT_POOL", "0")
    monkeypatch.setenv("ZRT_STACK_LDS_ROWS", "2")
    run = Run(scenes, 3, p)
    try:
        monkeypatch.setenv("ZRT_DEBUG_ROW_CAP", "0")
        run.begin()
        img = run.step(2)
        assert np.isnan(img).all()
        for call in (run.ctx.sync, run.ctx.stats, run.ctx.accum_info):
            with pytest.raises(z.ZrtError, match="past its buffer") as e:
                call()
            assert e.value.code == E_UNSUPPORTED
        monkeypatch.delenv("ZRT_DEBUG_ROW_CAP")
        with pytest.raises(z.ZrtError, match="past its buffer") as e:  # sticky: the accumulator is poisoned
            run.step(2)
        assert e.value.code == E_UNSUPPORTED
        run.begin()
        a = run.step(2)
        run.ctx.sync()
        b = run.step(2)
        run.ctx.sync()
        for img, spp in ((a, 2), (b, 4)):
            ref, rs = z.render(s, s.camera, dataclasses.replace(p, samples_per_pixel=spp))
            assert P.same_bits(img, ref).all() and np.isfinite(img).all()
        assert run.ctx.stats()["rays_processed"] == rs["rays_processed"]
    finally:
        run.close()


# ---- 7. one-shot and CLI ---------------------------------------------------------------

def test_render_progressive(scenes):
    """24 x 24, cap 12, pass_samples 3: four infos, z.render's image and stats; an on_pass
    that stops at its second call leaves the spp-6 frame and counters."""
    _, view, cam = E.scene_of(scenes, "wraps")
    p = E.frame_params(12, spp=12, chunk=3)
    full, fs = z.render(view, cam, p)
    seen = []
    img, st, infos = z.render_progressive(view, cam, p, pass_samples=3,
                                          on_pass=lambda im, info: seen.append(im.copy()) and False)
    assert [i["samples_done"] for i in infos] == [3, 6, 9, 12] and len(seen) == 4
    assert P.same_bits(img, full).all() and P.same_bits(seen[-1], full).all()
    for k in P.COUNTERS + ("sampling_loop", "used_bvh"):
        assert st[k] == fs[k], k
    ref6, rs6, _ = E.oracle_frame(scenes, "wraps", dataclasses.replace(p, samples_per_pixel=6))
    P.assert_bit_exact(seen[1], ref6)
    # pass_samples is rounded up to whole chunks (4 -> 6), and 0 selects the default (8 chunks)
    assert [i["samples_done"] for i in z.render_progressive(view, cam, p, pass_samples=4)[2]] == [6, 12]
    assert [i["samples_done"] for i in z.render_progressive(view, cam, p)[2]] == [12]
    p1 = dataclasses.replace(p, sample_chunk=1)
    assert [i["samples_done"] for i in z.render_progressive(view, cam, p1)[2]] == [8, 12]
    calls = []
    img, st, infos = z.render_progressive(view, cam, p, pass_samples=3,
                                          on_pass=lambda im, info: calls.append(info) or len(calls) == 2)
    assert [i["samples_done"] for i in infos] == [3, 6]
    P.assert_bit_exact(img, ref6)
    for k in P.COUNTERS:
        assert st[k] == rs6[k], k


def test_cli_pass_samples(tmp_path):
    """zrt-raytrace 32 32 8 5 1 out.png: ZRT_PASS_SAMPLES=4 (rounded up to the 32-sample
    chunk: one pass) and =0 write the PNG bytes of a run without it; a chunk-sized cap at
    64 spp prints two pass lines."""
    exe = os.path.join(z.REPO, "zraytrace_amd", "zrt-raytrace")
    env = {k: v for k, v in os.environ.items() if k not in ("ZRT_PASS_SAMPLES", "ZRT_DEVICES")}

    def cli(spp, out, **extra):
        r = subprocess.run([exe, "32", "32", str(spp), "5", "1", str(out)], env={**env, **extra},
                           capture_output=True, text=True, timeout=120)
        return r, [ln for ln in r.stderr.splitlines() if ln.startswith("Pass: ")]

    r0, l0 = cli(8, tmp_path / "plain.png")
    r1, l1 = cli(8, tmp_path / "prog.png", ZRT_PASS_SAMPLES="4")
    assert r0.returncode == 0 and r1.returncode == 0, r1.stderr
    assert (tmp_path / "plain.png").read_bytes() == (tmp_path / "prog.png").read_bytes()
    assert not l0 and len(l1) == 1 and "8 samples done" in l1[0]
    totals = [ln for ln in r0.stderr.splitlines() if ln.startswith("  Total ") and "runtime" not in ln]
    assert totals and totals == [ln for ln in r1.stderr.splitlines() if ln.startswith("  Total ") and "runtime" not in ln]
    r2, l2 = cli(64, tmp_path / "prog64.png", ZRT_PASS_SAMPLES="32")
    r3, _ = cli(64, tmp_path / "plain64.png")
    assert r2.returncode == 0 and len(l2) == 2 and "64 samples done" in l2[1], r2.stderr
    assert (tmp_path / "plain64.png").read_bytes() == (tmp_path / "prog64.png").read_bytes()
    r4, _ = cli(8, tmp_path / "both.png", ZRT_PASS_SAMPLES="4", ZRT_DEVICES="0")
    assert r4.returncode != 0 and "ZRT_PASS_SAMPLES" in r4.stderr and not (tmp_path / "both.png").exists()

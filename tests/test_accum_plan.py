"""The pass arithmetic of an accumulation run (zrt_debug_pass_plan; CPU only).

zrt_ctx_accum_pass renders samples [done, done + n) of a run capped at
samples_per_pixel as one launch of n samples whose sample keys are shifted by
`done` (planner.cpp plan_pass, the function the launch path itself calls).  Here
its plan is compared with a restatement in Python integers: the chunk
bookkeeping, the refusals, the bytes of chunk sums a pass parks, and the key
identity the shift rests on.
"""
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi

E_INVALID = _ffi.ZRT_E_INVALID


def params(cap, chunk, w=24, h=24, **kw):
    return z.RenderParams(w, h, cap, 4, sample_chunk=chunk, **kw)


def tiles_of(p):
    """This rank's 8x8 tiles: x in [0, height) (raytrace.zig:168's bound) by y in [0, height)."""
    n = ((p.height + 7) // 8) ** 2
    return (n - p.rank + p.world_size - 1) // p.world_size if n > p.rank else 0


def expect(p, done, n):
    """The plan restated; None where the run refuses the pass."""
    chunk = p.sample_chunk or 32
    if n == 0 or done + n > p.samples_per_pixel or done % chunk:
        return None
    chunks = -(-n // chunk)
    return {"first_sample": done, "pass_samples": n, "samples_after": done + n, "chunk": chunk,
            "pass_chunks": chunks, "last_chunk": n - (chunks - 1) * chunk,
            "partial_bytes": tiles_of(p) * 64 * chunks * 16, "key_offset": done}


def refused(p, done, n):
    with pytest.raises(z.ZrtError) as e:
        z.debug_pass_plan(p, done, n)
    assert e.value.code == E_INVALID
    return str(e.value)


def test_whole_chunk_passes():
    """chunk 3, cap 12, passes 3 / 6 / 3."""
    p = params(12, 3)
    done = 0
    for n, chunks in ((3, 1), (6, 2), (3, 1)):
        plan = z.debug_pass_plan(p, done, n)
        assert plan == expect(p, done, n)
        assert (plan["pass_chunks"], plan["last_chunk"], plan["key_offset"]) == (chunks, 3, done)
        done = plan["samples_after"]
    assert done == 12
    refused(p, 12, 1)


def test_ragged_pass_ends_the_run():
    """done 6, n 4, cap 10: chunks of 3 and 1 samples; nothing starts at sample 10 or at 7 .. 9."""
    p = params(10, 3)
    plan = z.debug_pass_plan(p, 6, 4)
    assert plan == expect(p, 6, 4)
    assert (plan["pass_chunks"], plan["last_chunk"], plan["samples_after"]) == (2, 1, 10)
    refused(p, 10, 1)
    # a ragged pass below the cap: the run cannot grow from a start that is no chunk boundary
    q = params(12, 3)
    assert z.debug_pass_plan(q, 6, 4)["last_chunk"] == 1
    assert "chunk boundary" in refused(q, 10, 2)


def test_refusals():
    p = params(12, 3)
    assert "0 samples" in refused(p, 0, 0)
    assert "past" in refused(p, 9, 4)
    assert "past" in refused(p, 0, 13)
    assert "chunk boundary" in refused(p, 4, 3)
    assert "u16" in refused(params(65536, 3), 0, 3)  # cap > 65535: RenderParams fields are u16
    for done, n in ((0, 0), (9, 4), (4, 3), (0, 12), (3, 9), (2, 1)):
        if expect(p, done, n) is None:
            refused(p, done, n)
        else:
            assert z.debug_pass_plan(p, done, n) == expect(p, done, n)


def test_chunk_zero_selects_32():
    p = params(256, 0)
    plan = z.debug_pass_plan(p, 64, 100)
    assert plan == expect(p, 64, 100)
    assert (plan["chunk"], plan["pass_chunks"], plan["last_chunk"]) == (32, 4, 4)
    refused(p, 16, 32)


@pytest.mark.parametrize("w,h", [(20, 13), (13, 20)])
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 3)])
def test_partial_bytes(w, h, rank, world):
    """tiles x 64 x pass_chunks x 16 B, the tiles covering x < height (the reference's
    bound) - a pass's need, not the frame's.  height > width is refused as everywhere."""
    p = params(12, 3, w=w, h=h, rank=rank, world_size=world)
    if h > w:
        assert "height > width" in refused(p, 0, 6)
        return
    assert tiles_of(p) == {(0, 1): 4, (1, 3): 1}[rank, world]
    for done, n in ((0, 3), (0, 6), (6, 4), (0, 12)):
        plan = z.debug_pass_plan(p, done, n)
        assert plan == expect(p, done, n)
        assert plan["partial_bytes"] == tiles_of(p) * 64 * plan["pass_chunks"] * 16


def test_last_plan_reaches_sample_65534():
    p = params(65535, 4096, w=2, h=2)
    a = z.debug_pass_plan(p, 0, 61440)
    assert a == expect(p, 0, 61440) and a["pass_chunks"] == 15
    b = z.debug_pass_plan(p, 61440, 4095)
    assert b == expect(p, 61440, 4095)
    assert (b["pass_chunks"], b["last_chunk"], b["samples_after"]) == (1, 4095, 65535)
    assert b["first_sample"] + b["pass_samples"] - 1 == 65534  # the last sample index of a u16 spp
    refused(p, 65535, 1)


def test_key_identity():
    """((o << 16) | s) + s0 == (o << 16) | (s + s0) while s + s0 < 65536: the shift added
    to the seed term reaches the frame's sample s + s0, at the top of both ranges (the
    last pixel of a 65535 x 65535 frame, the last sample of a u16 count)."""
    o = 65534 * 65535 + 65534
    mix = (42 * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    for s, s0 in ((0, 65535), (65535, 0), (4094, 61441), (1, 0), (0, 0)):
        assert s + s0 < 65536
        assert ((o << 16) | s) + s0 == (o << 16) | (s + s0)
        # with the seed term, in the kernel's 64-bit arithmetic
        assert ((((o << 16) | s) + ((mix + s0) & (2 ** 64 - 1))) & (2 ** 64 - 1) ==
                (((o << 16) | (s + s0)) + mix) & (2 ** 64 - 1))

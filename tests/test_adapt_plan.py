"""The level list of an adaptive run (zrt_debug_adapt_plan; CPU only).

zrt_ctx_adapt_begin takes its sample levels from planner.cpp plan_adapt, the
function zrt_debug_adapt_plan reports: L_0 = first_level in whole sample chunks
(at least one), doubled while below the cap, then the cap itself (zrt.h,
"adaptive sampling").  Here the list is compared with a restatement in Python
integers, and the refusals with the ones the header names.
"""
import ctypes as C
import math
import os
import subprocess

import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi

E_INVALID = _ffi.ZRT_E_INVALID

NEW_EXPORTS = ["zrt_ctx_adapt_begin", "zrt_ctx_adapt_level", "zrt_ctx_adapt_samples", "zrt_render_adaptive",
               "zrt_render_adaptive_progress", "zrt_debug_adapt_plan"]


def params(cap, chunk, w=24, h=24, **kw):
    return z.RenderParams(w, h, cap, 4, sample_chunk=chunk, **kw)


def expect(cap, chunk, first):
    chunk = chunk or 32
    level = max(1, -(-first // chunk)) * chunk
    out = []
    while level < cap:
        out.append(level)
        level *= 2
    return out + [cap]


def test_doubling_levels():
    assert z.adapt_plan(params(12, 3), 0.5, 3) == [3, 6, 12]
    assert z.adapt_plan(params(48, 3), 0.5, 3) == [3, 6, 12, 24, 48]
    assert z.adapt_plan(params(1024, 0), 0.0, 32) == [32, 64, 128, 256, 512, 1024]


def test_ragged_last_level():
    """cap 20, chunk 3: 24 is not below the cap, so the cap ends the list (7 chunks, the last of 2 samples)."""
    assert z.adapt_plan(params(20, 3), 0.5, 3) == [3, 6, 12, 20]
    assert z.debug_pass_plan(params(20, 3), 12, 8)["last_chunk"] == 2


def test_first_level_rounds_up_to_chunks():
    assert z.adapt_plan(params(48, 3), 0.5, 4) == [6, 12, 24, 48]
    assert z.adapt_plan(params(48, 3), 0.5, 0) == [3, 6, 12, 24, 48]  # 0: one chunk
    assert z.adapt_plan(params(64, 0), 0.5, 1) == [32, 64]             # chunk 0 selects 32


def test_first_level_at_or_past_the_cap():
    for first in (12, 13, 48, 2 ** 32 - 1):
        assert z.adapt_plan(params(12, 3), 0.5, first) == [12]
    assert z.adapt_plan(params(2, 3), 0.5, 0) == [2]  # (one chunk is already past the cap)


@pytest.mark.parametrize("cap", [1, 5, 31, 32, 33, 100, 1000, 65535])
@pytest.mark.parametrize("chunk", [0, 1, 3, 7, 4096])
@pytest.mark.parametrize("first", [0, 1, 5, 64, 5000])
def test_levels_against_the_restatement(cap, chunk, first):
    got = z.adapt_plan(params(cap, chunk, w=8, h=8), 0.25, first)
    assert got == expect(cap, chunk, first)
    c = chunk or 32
    assert all(level % c == 0 for level in got[:-1])  # every level but the last ends on a chunk boundary
    assert len(got) <= max(0.0, math.log2(cap / got[0])) + 2
    # every level is a pass the run accepts
    done = 0
    for level in got:
        assert z.debug_pass_plan(params(cap, chunk, w=8, h=8), done, level - done)["samples_after"] == level
        done = level


@pytest.mark.parametrize("tol", [-1.0, -1e-30, float("nan"), float("inf"), -float("inf")])
def test_tolerance_refusals(tol):
    with pytest.raises(z.ZrtError) as e:
        z.adapt_plan(params(12, 3), tol, 3)
    assert e.value.code == E_INVALID and "tolerance" in str(e.value)


def test_tolerance_zero_and_large_are_accepted():
    assert z.adapt_plan(params(12, 3), 0.0, 3) == [3, 6, 12]
    assert z.adapt_plan(params(12, 3), 1e30, 3) == [3, 6, 12]


def test_null_arguments():
    L = z.lib()
    p = params(12, 3).abi()
    ad = _ffi.Adaptive(tolerance=0.5, first_level=3)
    levels = (C.c_uint32 * 8)()
    n = C.c_uint32()
    assert L.zrt_debug_adapt_plan(None, C.byref(ad), levels, 8, C.byref(n)) == E_INVALID
    assert L.zrt_debug_adapt_plan(C.byref(p), None, levels, 8, C.byref(n)) == E_INVALID
    assert L.zrt_debug_adapt_plan(C.byref(p), C.byref(ad), None, 8, C.byref(n)) == E_INVALID
    assert L.zrt_debug_adapt_plan(C.byref(p), C.byref(ad), levels, 8, None) == E_INVALID
    # a short buffer takes the first entries; the count is the whole list's
    assert L.zrt_debug_adapt_plan(C.byref(p), C.byref(ad), levels, 2, C.byref(n)) == 0
    assert (n.value, list(levels[:3])) == (3, [3, 6, 0])
    assert L.zrt_debug_adapt_plan(C.byref(p), C.byref(ad), None, 0, C.byref(n)) == 0 and n.value == 3


def test_what_a_pass_refuses():
    """The cap goes through plan_pass: the 16-bit sample index, a tall frame, a rank past the world."""
    for bad in (params(65536, 3), params(0, 3), params(12, 3, w=13, h=20), params(12, 3, rank=2, world_size=2),
                params(12, 65536)):
        with pytest.raises(z.ZrtError) as e:
            z.adapt_plan(bad, 0.5, 3)
        assert e.value.code == E_INVALID
        with pytest.raises(z.ZrtError):
            z.debug_pass_plan(bad, 0, bad.samples_per_pixel)


def test_exports_present():
    lib = os.path.join(z.REPO, "zraytrace_amd", "libzrt.so")
    names = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in names.splitlines() if ln.strip()}
    for name in NEW_EXPORTS:
        assert name in exported, name
        assert any(sig[0] == name for sig in _ffi.SIGNATURES), name

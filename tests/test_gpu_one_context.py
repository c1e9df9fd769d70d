"""One context, every feature in turn.

The other suites cover each feature of a context alone.  This one runs them one
after the other on a single context - a plain frame, a three-pass accumulation run
with a feature launch between two of its passes, a second accum_begin while passes
of an abandoned run are still pending, the variance plane, an adaptive run to its
last level, a plain frame (which ends the run: a variance call is then refused), a
guided denoise, and two temporal steps of which the second has another frame size -
and compares every output, bit for bit, and the counters of zrt_ctx_stats with those
of a fresh context that performs that step alone: no state of one feature may
survive into another.

Scene 2 (the bunny), FAST traversal: at test_gpu_progressive's ragged 20 x 13 frame
(12 samples in chunks of 3), and at test_gpu_order_cache's 64 x 64 x 128, where the
scheduling probe and the kept tile order take part (the shared context reuses the
order its first frame left, a fresh one probes).

Run on an MI355X: ``pytest -m gpu``.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z

pytestmark = pytest.mark.gpu

E_INVALID = z._ffi.ZRT_E_INVALID


@dataclasses.dataclass
class Case:
    p: z.RenderParams
    passes: tuple       # the three passes of a run
    first_level: int    # of the adaptive run
    small: tuple        # (width, height) of the second temporal step


CASES = {
    "ragged-12": Case(z.RenderParams(20, 13, 12, 8, sample_chunk=3), (6, 3, 3), 3, (16, 10)),
    "scheduled-128": Case(z.RenderParams(64, 64, 128, 6, sample_chunk=16), (48, 48, 32), 16, (48, 40)),
}


def dev(n, fill=None):
    import torch
    if fill is None:
        return torch.zeros(n, dtype=torch.float32, device="cuda")
    return torch.full((n,), fill, dtype=torch.float32, device="cuda")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).copy()


def counters(ctx):
    """zrt_ctx_stats without its times."""
    return {k: v for k, v in ctx.stats().items() if not k.endswith("_ms")}


def tiles_of(ctx, p):
    return dev(ctx.tile_count(p) * 64 * 3)


def plain_frame(ctx, cam, k, seed=42):
    p = dataclasses.replace(k.p, seed=seed)
    t = tiles_of(ctx, p)
    ctx.render_tiles(cam, p, t.data_ptr())
    return {"tiles": host(t), "stats": counters(ctx)}


def run_with_features(ctx, cam, k):
    """Three passes, nothing waited for in between, a feature launch after the first."""
    t, f = tiles_of(ctx, k.p), dev(k.p.width * k.p.height * 8)
    ctx.accum_begin(cam, k.p)
    ctx.accum_pass(k.passes[0], t.data_ptr())
    ctx.features(cam, k.p, f.data_ptr())
    ctx.accum_pass(k.passes[1], t.data_ptr())
    ctx.accum_pass(k.passes[2], t.data_ptr())
    out = {"tiles": host(t), "features": host(f), "stats": counters(ctx)}
    info = ctx.accum_info()
    out["info"] = {n: info[n] for n in ("samples_done", "pass_samples", "changed_pixels")}
    ctx.sync()
    return out


def second_run_and_variance(ctx, cam, k, abandon):
    """abandon: two passes of a run first, left pending (neither waited for nor read).
    Then a run with another seed, two passes, its variance plane."""
    q = dataclasses.replace(k.p, seed=7)
    t, v = tiles_of(ctx, q), dev(ctx.tile_count(q) * 64)
    if abandon:
        gone = tiles_of(ctx, k.p)
        ctx.accum_begin(cam, k.p)
        ctx.accum_pass(k.passes[0], gone.data_ptr())
        ctx.accum_pass(k.passes[1], gone.data_ptr())
    ctx.accum_begin(cam, q)
    ctx.accum_pass(k.passes[0], t.data_ptr())
    ctx.accum_pass(k.passes[1], t.data_ptr())
    ctx.accum_variance(v.data_ptr())
    return {"tiles": host(t), "variance": host(v), "stats": counters(ctx)}


def adaptive_run(ctx, cam, k):
    t, v = tiles_of(ctx, k.p), dev(ctx.tile_count(k.p) * 64)
    ctx.adapt_begin(cam, k.p, 0.05, k.first_level)
    levels = []
    for _ in z.adapt_plan(k.p, 0.05, k.first_level):
        info = ctx.adapt_level(t.data_ptr())
        levels.append({n: info[n] for n in ("level_samples", "tiles_rendered", "tiles_active_after",
                                            "samples_rendered", "changed_pixels")})
        if info["tiles_active_after"] == 0:
            break
    ctx.accum_variance(v.data_ptr())
    return {"tiles": host(t), "variance": host(v), "levels": levels, "per_tile": ctx.adapt_samples().copy(),
            "stats": counters(ctx)}


def rendered(ctx, cam, p):
    """A plain frame of p, assembled, with its features: (frame, features) on the device."""
    t, frame, f = tiles_of(ctx, p), dev(p.width * p.height * 3), dev(p.width * p.height * 8)
    ctx.render_tiles(cam, p, t.data_ptr())
    ctx.assemble(p, t.data_ptr(), frame.data_ptr())
    ctx.features(cam, p, f.data_ptr())
    return frame, f


def guided_denoise(ctx, cam, k):
    p = k.p
    frame, f = rendered(ctx, cam, p)
    var, out, out_var = dev(p.width * p.height, 0.01), dev(p.width * p.height * 3), dev(p.width * p.height)
    dn, flags = z.denoise_guided_defaults()
    ctx.denoise_guided(p, dn, flags, frame.data_ptr(), f.data_ptr(), var.data_ptr(), out.data_ptr(), out_var.data_ptr())
    res = {"out": host(out), "out_variance": host(out_var), "stats": counters(ctx)}
    ctx.sync()
    assert ctx.denoise_ms() > 0
    return res


def temporal_pair(ctx, cam, k):
    res = {}
    tp = z.temporal_defaults()
    small = dataclasses.replace(k.p, width=k.small[0], height=k.small[1])
    for name, p, seed in (("first", k.p, 42), ("second", small, 43)):
        p = dataclasses.replace(p, seed=seed)
        n = p.width * p.height
        frame, f = rendered(ctx, cam, p)
        import torch
        var, out, out_var = dev(n, 0.01), dev(n * 3), dev(n)
        out_len = torch.zeros(n, dtype=torch.int32, device="cuda")
        ctx.temporal(cam, p, tp, frame.data_ptr(), f.data_ptr(), var.data_ptr(), out.data_ptr(), out_var.data_ptr(),
                     out_len.data_ptr())
        res[name] = host(out)
        res[name + "_variance"] = host(out_var)
        res[name + "_len"] = out_len.cpu().numpy().copy()
        res[name + "_stats"] = counters(ctx)
    ctx.sync()
    assert ctx.temporal_ms() > 0
    return res


def same(a, b, where):
    assert type(a) is type(b), where
    if isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for n in a:
            same(a[n], b[n], where + "/" + str(n))
    elif isinstance(a, list):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, where + "/" + str(i))
    elif isinstance(a, np.ndarray):
        np.testing.assert_array_equal(a, b, err_msg=where)
    else:
        assert a == b, where


@pytest.mark.parametrize("case", list(CASES))
def test_every_feature_in_turn(scenes, case, monkeypatch):
    monkeypatch.delenv("ZRT_ORDER_CACHE", raising=False)
    k = CASES[case]
    s = scenes(2)
    cam = s.camera
    steps = [
        ("plain frame", lambda c, shared: plain_frame(c, cam, k)),
        ("run with features", lambda c, shared: run_with_features(c, cam, k)),
        ("second run, variance", lambda c, shared: second_run_and_variance(c, cam, k, abandon=shared)),
        ("adaptive run", lambda c, shared: adaptive_run(c, cam, k)),
        ("plain frame ends the run", lambda c, shared: plain_frame(c, cam, k, seed=9)),
        ("guided denoise", lambda c, shared: guided_denoise(c, cam, k)),
        ("temporal pair", lambda c, shared: temporal_pair(c, cam, k)),
    ]
    got = {}
    ctx = z.RenderContext(s, k.p)
    try:
        for name, step in steps:
            got[name] = step(ctx, True)
            if name == "plain frame ends the run":
                with pytest.raises(z.ZrtError) as e:
                    ctx.accum_variance(dev(ctx.tile_count(k.p) * 64).data_ptr())
                assert e.value.code == E_INVALID and "no run is live" in str(e.value)
    finally:
        ctx.close()
    for name, step in steps:
        ctx = z.RenderContext(s, k.p)
        try:
            alone = step(ctx, False)
        finally:
            ctx.close()
        same(got[name], alone, case + ": " + name)

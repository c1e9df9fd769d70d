"""GPU tests of the runtime around the kernel: device-error surfacing, stream
semantics of the C ABI, the persistent multi-GPU context, and bench.py's N-rank
step (render_tiles -> gather -> assemble) end to end.

Run on an MI355X: ``pytest -m gpu``.
"""
import os
import socket

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu

COUNTERS = ("recursion_depth_hits", "reflections", "background_hits", "rays_processed",
            "pixels_processed", "samples_processed")


def same_bits(a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


# ---- device errors surface without a stats call (raytrace.zig:136-138's error union) ---

@pytest.mark.parametrize("traversal", [z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE, z.ZRT_TRAVERSAL_BINARY],
                         ids=["fast", "reference", "binary"])
def test_stack_overflow_is_an_error(scenes, traversal, monkeypatch):
    """A traversal stack too small for the tree (forced by ZRT_DEBUG_STACK_CAP):
    zrt_render returns ZRT_E_UNSUPPORTED instead of a silently wrong frame."""
    monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
    s = scenes(3)  # teapot: reference BVH depth > 4
    with pytest.raises(z.ZrtError) as e:
        z.render(s, s.camera, z.RenderParams(32, 32, 2, 8, traversal=traversal))
    assert e.value.code == z._ffi.ZRT_E_UNSUPPORTED
    assert "overflow" in str(e.value)


def test_stack_overflow_context_path(scenes, monkeypatch):
    """The asynchronous path: the launch's tiles are NaN, zrt_ctx_sync reports the
    error, and a caller that never synchronises through the ABI gets it from the
    next zrt_ctx_render_tiles (once); after that the context renders correctly."""
    import torch
    s = scenes(3)
    p = z.RenderParams(32, 32, 2, 8)
    ctx = z.RenderContext(s, p)
    buf = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
    monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
    ctx.render_tiles(s.camera, p, buf.data_ptr())
    with pytest.raises(z.ZrtError) as e:
        ctx.sync()
    assert e.value.code == z._ffi.ZRT_E_UNSUPPORTED
    assert torch.isnan(buf).all()
    # a caller that skipped sync: the next launch reports the finished one's error, once
    ctx.render_tiles(s.camera, p, buf.data_ptr())
    torch.cuda.synchronize()
    monkeypatch.delenv("ZRT_DEBUG_STACK_CAP")
    with pytest.raises(z.ZrtError) as e:
        ctx.render_tiles(s.camera, p, buf.data_ptr())
    assert e.value.code == z._ffi.ZRT_E_UNSUPPORTED
    ctx.render_tiles(s.camera, p, buf.data_ptr())
    ctx.sync()
    assert torch.isfinite(buf).all()
    ctx.close()


def test_render_tiles_rejects_mismatched_params(scenes):
    s = scenes(2)
    p = z.RenderParams(16, 16, 1, 4)
    ctx = z.RenderContext(s, p)
    import torch
    buf = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
    for bad in (z.RenderParams(16, 16, 1, 4, device=1), z.RenderParams(16, 16, 1, 4, bounded_volume_hierarchy=False)):
        with pytest.raises(z.ZrtError) as e:
            ctx.render_tiles(s.camera, bad, buf.data_ptr())
        assert e.value.code == z._ffi.ZRT_E_INVALID
    ctx.close()


# ---- stream semantics (zrt.h: NULL = the context's blocking stream) ----------------

def test_null_stream_orders_before_torch_default_stream(scenes):
    """Tiles rendered on the NULL stream (the context's own, blocking stream) are
    complete when the next work on torch's default (legacy) stream reads them,
    with no host synchronisation in between."""
    import torch
    s = scenes(2)
    p = z.RenderParams(256, 256, 64, 20)
    ref, _ = z.render(s, s.camera, p)
    ctx = z.RenderContext(s, p)
    n = ctx.tile_count(p)
    tiles = torch.full((n * 64 * 3,), -1.0, dtype=torch.float32, device="cuda")
    frame = torch.empty(256 * 256 * 3, dtype=torch.float32, device="cuda")
    for _ in range(3):
        tiles.fill_(-1.0)
        ctx.render_tiles(s.camera, p, tiles.data_ptr(), 0)
        copy = tiles.clone()  # torch's default stream: must see the finalized tiles
        ctx.assemble(p, copy.data_ptr(), frame.data_ptr(), 0)
        torch.cuda.synchronize()
        assert same_bits(frame.cpu().numpy().reshape(256, 256, 3), ref)
    ctx.close()


# ---- persistent multi-GPU context ----------------------------------------------------

@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_multi_context_frames(scenes, devices):
    """zrt_multi_*: scene uploaded once, several frames with different params;
    every frame equals zrt_render's (and counters sum to it)."""
    s = scenes(2)
    m = z.MultiContext(s, z.RenderParams(40, 40, 4, 20), devices)
    for w, h, spp in ((40, 40, 4), (24, 16, 8), (40, 40, 4)):
        p = z.RenderParams(w, h, spp, 20)
        one, st1 = z.render(s, s.camera, p)
        img, stm = m.render(s.camera, p)
        assert same_bits(one, img)
        for k in COUNTERS:
            assert st1[k] == stm[k], k
        assert stm["n_gpus"] == 1
        # the frame left on devices[0] (out_rgb NULL) and read back later is the same
        none, stk = m.render(s.camera, p, copy_out=False)
        assert none is None and stk["rays_processed"] == st1["rays_processed"]
        assert same_bits(m.frame(), one)
        ms = m.rank_ms()
        assert len(ms) == len(devices) and all(x > 0 for x in ms)
    m.close()


def test_bench_one_process_rehearsal(scenes):
    """bench.py's one-process path (no launcher: zrt_multi_*) rehearsed with two
    ranks on GPU 0 (--devices 0,0): one JSON line whose frame is zrt_render's bit
    for bit, with each rank's kernel time."""
    import hashlib
    import json
    import subprocess
    import sys
    s = scenes(2)
    one, st1 = z.render(s, s.camera, z.RenderParams(96, 80, 8, 20))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"),
                        "--devices", "0,0", "--steps", "2", "--warmup", "1", "--width", "96", "--height", "80",
                        "--spp", "8"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["frame_sha1"] == hashlib.sha1(one.tobytes()).hexdigest()
    assert line["n_gpus"] == 1 and line["ranks"] == 2 and len(line["per_rank_ms"]["kernel"]) == 2
    assert line["rays_per_step"] == st1["rays_processed"]
    assert line["value"] > 0


def test_bench_plain_run_dumps_its_frame(scenes, tmp_path):
    """A plain bench.py run (no --full) times its steps and stops: no STATS launch, so
    no roofline, reference-traversal or CPU-baseline fields; --dump-outputs writes the
    last timed frame and its counters, equal to zrt_render's bit for bit."""
    import json
    import subprocess
    import sys
    s = scenes(2)
    one, st1 = z.render(s, s.camera, z.RenderParams(96, 80, 8, 20))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"),
                        "--gpus", "1", "--steps", "3", "--warmup", "1", "--width", "96", "--height", "80",
                        "--spp", "8", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["steps"] == 3 and r.stderr.count("/3: kernel ") == 3
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "Mrays/s" and line["dtype"] == "f32"
    assert line["rays_per_step"] == st1["rays_processed"]
    assert line["full"] is False
    assert not {"roofline", "simd", "reference_traversal", "cpu_baseline"} & set(line)
    assert sorted(os.listdir(tmp_path)) == ["counters.npy", "frame.npy"]
    frame = np.load(tmp_path / "frame.npy")
    assert frame.dtype == np.float32 and same_bits(frame, one)
    counters = np.load(tmp_path / "counters.npy")
    order = ("recursion_depth_hits", "reflections", "background_hits", "pixels_processed", "samples_processed",
             "rays_processed")  # bench.PROGRESS_COUNTERS
    assert counters.dtype == np.float64 and [int(x) for x in counters] == [st1[k] for k in order]


def test_bench_full_adds_the_stats_report(scenes):
    """bench.py --full: the same line plus what the untimed ZRT_FLAG_STATS launch
    counted (roofline with its algorithmic bytes, simd, accel) and the REFERENCE-
    traversal frame, equal to FAST's (the CPU baseline, ~15 s of one core, left out)."""
    import json
    import subprocess
    import sys
    s = scenes(2)
    _, st1 = z.render(s, s.camera, z.RenderParams(96, 80, 8, 20))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"),
                        "--gpus", "1", "--steps", "1", "--warmup", "0", "--width", "96", "--height", "80",
                        "--spp", "8", "--full", "--no-cpu-baseline"], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["full"] is True and line["rays_per_step"] == st1["rays_processed"]
    assert line["roofline"]["algorithmic"]["bytes_per_launch"] > 0
    assert "ZRT_FLAG_STATS" in line["roofline"]["counters_from"]
    assert line["simd"]["sampling_loop"] != "unknown" and line["accel"]["wide_nodes"] > 0
    assert line["reference_traversal"]["frame_equal_to_fast"] is True
    assert line["reference_traversal"]["rays"] == st1["rays_processed"]
    assert "cpu_baseline" not in line


def test_multi_render_surfaces_device_error(scenes, monkeypatch):
    monkeypatch.setenv("ZRT_DEBUG_STACK_CAP", "4")
    s = scenes(3)
    with pytest.raises(z.ZrtError) as e:
        z.render_multi(s, s.camera, z.RenderParams(24, 24, 1, 6), [0, 0])
    assert e.value.code == z._ffi.ZRT_E_UNSUPPORTED


# ---- bench.py's N-rank step, end to end ---------------------------------------------

def _free_port():
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def _rank_worker(rank, world, port, scene_index, dims, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import zraytrace_amd as zz
        from zraytrace_amd.dist import TileFrame
        s = zz.load_scene(scene_index)
        w, h, spp, depth = dims
        p = zz.RenderParams(w, h, spp, depth, rank=rank, world_size=world, device=0)
        fr = TileFrame(s, p, rank, world)
        for _ in range(2):  # the buffers are reused across steps
            fr.step()
        st = fr.ctx.stats()
        img = fr.image() if rank == 0 else None
        q.put((rank, img, {k: st[k] for k in COUNTERS}))
        fr.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_tileframe_ranks_end_to_end(scenes, world):
    """world gloo ranks sharing GPU 0 run bench.py's step (TileFrame: render_tiles
    on an explicit stream -> padded gather -> assemble_padded): rank 0's frame
    equals zrt_render's and the oracle's bit for bit, and the ranks' counters sum
    to zrt_render's."""
    import torch.multiprocessing as mp
    dims = (40, 40, 4, 20)
    s = scenes(2)
    p = z.RenderParams(*dims)
    one, st1 = z.render(s, s.camera, p)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, 2, dims, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    got = [q.get(timeout=240) for _ in range(world)]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    img = next(g[1] for g in got if g[0] == 0)
    assert same_bits(img, one)
    ref, _ = O.render(s.view, s.camera, p)
    assert same_bits(img, ref)
    for k in COUNTERS:
        assert sum(g[2][k] for g in got) == st1[k], k


# ---- per-scanline Progress counters (raytrace.zig:37-50, 184; ZRT_FLAG_SCANLINES) ----

@pytest.mark.parametrize("scene_index,dims", [(1, (40, 24, 4, 30)), (2, (48, 40, 8, 20)), (3, (33, 33, 2, 20))],
                         ids=["list", "bunny", "teapot-ragged"])
def test_scanlines_match_oracle(scenes, scene_index, dims):
    """zrt_render_progress: every row's counters equal the deltas the oracle
    records after each scanline (the reference's printProgress), the image is
    zrt_render's, and the rows sum to the frame's counters."""
    s = scenes(scene_index)
    p = z.RenderParams(*dims)
    img, st, rows = z.render_progress(s, s.camera, p)
    plain, st0 = z.render(s, s.camera, p)
    ref, rst, rrows = O.render_scanlines(s.view, s.camera, p)
    assert same_bits(img, plain) and same_bits(img, ref)
    np.testing.assert_array_equal(rows, rrows)
    tot = rows.sum(axis=0)
    for i, k in enumerate(("recursion_depth_hits", "reflections", "background_hits", "pixels_processed",
                           "samples_processed", "rays_processed")):
        assert tot[i] == st[k] == st0[k] == rst[k], k


def test_scanlines_over_ranks(scenes):
    """Per-rank contexts (tiles round-robin) with ZRT_FLAG_SCANLINES: the ranks'
    rows sum to the oracle's; a MultiContext sums them itself; a launch without
    the flag has no rows to read."""
    s = scenes(2)
    w, h, spp, depth = 40, 32, 4, 20
    _, _, rrows = O.render_scanlines(s.view, s.camera, z.RenderParams(w, h, spp, depth))
    import torch
    total = np.zeros_like(rrows)
    for r in range(3):
        p = z.RenderParams(w, h, spp, depth, rank=r, world_size=3, flags=z.ZRT_FLAG_SCANLINES)
        ctx = z.RenderContext(s, p)
        buf = torch.zeros(max(1, ctx.tile_count(p)) * 64 * 3, dtype=torch.float32, device="cuda")
        ctx.render_tiles(s.camera, p, buf.data_ptr())
        total += ctx.scanlines(h)
        ctx.render_tiles(s.camera, z.RenderParams(w, h, spp, depth, rank=r, world_size=3), buf.data_ptr())
        with pytest.raises(z.ZrtError):
            ctx.scanlines(h)
        ctx.close()
    np.testing.assert_array_equal(total, rrows)
    m = z.MultiContext(s, z.RenderParams(w, h, spp, depth), [0, 0])
    m.render(s.camera, z.RenderParams(w, h, spp, depth, flags=z.ZRT_FLAG_SCANLINES))
    np.testing.assert_array_equal(m.scanlines(h), rrows)
    m.close()


# ---- the reference BVH built on the GPU (bvh_gpu.hip; bvh.zig:62-185) ---------------

def _same_tree(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert x.shape == y.shape
        assert (np.ascontiguousarray(x).view(np.uint32) == np.ascontiguousarray(y).view(np.uint32)).all()
    assert a[4] == b[4]


@pytest.mark.parametrize("index", [0, 2, 3, 4])
def test_device_bvh_matches_host_and_oracle(scenes, index):
    """Node for node (boxes bit for bit, children, leaf order, depth) the tree
    of the host build and of the oracle's comparison-sort restatement."""
    s = scenes(index)
    d = z.bvh_build_device(s)
    _same_tree(d, z.bvh_build(s))
    _same_tree(d, O.bvh_build(s.view))


@pytest.mark.parametrize("n,seed", [(3, 5), (4, 6), (50, 1), (3000, 2), (20000, 3), (70000, 4)])
def test_device_bvh_ties(n, seed):
    """Lattice scenes full of equal midpoints and signed zeros (test_host.py's
    generator): the segmented radix sorts keep the reference's tie order."""
    import ctypes as C
    from test_host import _synthetic_scene
    s = _synthetic_scene(n, seed)
    d = z.bvh_build_device(C.pointer(s))
    _same_tree(d, z.bvh_build(C.pointer(s)))
    if n <= 3000:
        _same_tree(d, O.bvh_build(C.pointer(s)))


def test_device_bvh_c5_substitute(scenes):
    """The 1.6 M-triangle C5 substitute: the device build equals the host
    build node for node (1 894 803 nodes, depth 39) and is much faster."""
    import time
    s = scenes(6)
    t0 = time.time()
    d = z.bvh_build_device(s)
    t1 = time.time()
    h = z.bvh_build(s)
    t2 = time.time()
    _same_tree(d, h)
    assert (len(d[0]), d[4]) == (1894803, 39)
    print(f"device build {t1 - t0:.3f} s, host build {t2 - t1:.3f} s")
    assert t1 - t0 < (t2 - t1) / 3


def test_device_bvh_failure_falls_back_to_host(scenes, monkeypatch):
    """a HIP failure inside the device BVH build (forced here with
    ZRT_DEBUG_BVH_DEVICE_FAIL) makes zrt_bvh_build_device fail with ZRT_E_HIP,
    while zrt_render falls back to the host build of the same tree: the frame
    and counters equal those of a host-built context."""
    s = scenes(2)
    p = z.RenderParams(24, 24, 2, 8)
    monkeypatch.setenv("ZRT_BVH_DEVICE", "0")
    ref, rst = z.render(s, s.camera, p)
    monkeypatch.setenv("ZRT_BVH_DEVICE", "1")
    monkeypatch.setenv("ZRT_DEBUG_BVH_DEVICE_FAIL", "1")
    with pytest.raises(z.ZrtError) as e:
        z.bvh_build_device(s)
    assert e.value.code == _ffi.ZRT_E_HIP
    img, st = z.render(s, s.camera, p)
    assert (img.view(np.uint32) == ref.view(np.uint32)).all()
    assert st["rays_processed"] == rst["rays_processed"]


@pytest.mark.parametrize("scene_index,env,loop", [(1, {}, 6), (1, {"ZRT_LIST_LANES": "0"}, 0), (2, {}, 3),
                                                  (2, {"ZRT_WF": "1", "ZRT_POOL": "0"}, 4),
                                                  (2, {"ZRT_POOL": "1"}, 5), (6, {}, 5)])
def test_stats_report_the_sampling_loop(scenes, scene_index, env, loop, monkeypatch):
    """zrt_stats.sampling_loop names the loop the launch ran: the
    surface list with per-lane work items for the 7 spheres (the wave-unit list
    loop when ZRT_LIST_LANES=0), the lockstep loop for the bunny, the path pool
    for the 1.6 M-triangle C5 mesh (a tree past the 16-bit stack), and the loops
    ZRT_WF / ZRT_POOL force."""
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_LIST_LANES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = scenes(scene_index)
    _, st = z.render(s, s.camera, z.RenderParams(16, 16, 1, 4))
    assert st["sampling_loop"] == loop


def test_distant_camera_triangle_scene_does_not_replay(scenes):
    """in a scene without spheres no ray needs the
    sphere-slot origin bound, so a camera far outside the scene's box no longer
    sends every ray to the reference replay.  The bunny's triangles alone (no
    ground sphere) seen from 30x the model's size away: the frame equals the
    oracle's bit for bit and order replays stay a tiny fraction of the rays."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import hazard_rays as H
    from test_gpu_parity import prim_array
    pr = prim_array(scenes(2).view.contents)
    tri = pr[pr["kind"] == _ffi.ZRT_PRIM_TRIANGLE]
    scene = H.scene_of([], [(t["a"], t["b"], t["c"]) for t in tri])
    pts = np.concatenate([tri["a"], tri["b"], tri["c"]]).reshape(-1, 3)
    ctr = (pts.min(0) + pts.max(0)) / 2
    size = float(np.max(pts.max(0) - pts.min(0)))
    cam = z.camera_init(ctr + np.array([0.3, 0.2, 30.0]) * size, ctr, (0, 1, 0), 2.5, 1.0)
    p = z.RenderParams(48, 48, 4, 4, flags=z.ZRT_FLAG_STATS)
    img, st = z.render(scene, cam, p)
    ref, rs = O.render(scene, cam, p)
    assert same_bits(img, ref)
    assert st["rays_processed"] == rs["rays_processed"]
    assert st["order_replays"] <= 0.01 * st["rays_processed"], st["order_replays"]


@pytest.mark.parametrize("loop", ["wavefront", "pool"])
def test_scheduled_launch_of_other_loops(scenes, loop, monkeypatch):
    """The scheduling probe (a lockstep launch with its own LDS plan, spp >= 128)
    in front of a wavefront / path-pool render on a frame large enough that the
    probe's grid equals the render's (> 4096 tiles): the probe's global
    attenuation and stack rows fit the buffers it shares with the render launch
    (round 5: the wavefront render's 12 LDS rows left the probe's rows 2x too few),
    and the frame equals the lockstep loop's bit for bit."""
    s = scenes(3)
    p = z.RenderParams(640, 640, 128, 20)
    monkeypatch.setenv("ZRT_WF", "0")
    monkeypatch.setenv("ZRT_POOL", "0")
    ref, rs = z.render(s, s.camera, p)
    monkeypatch.setenv("ZRT_WF", "1" if loop == "wavefront" else "0")
    monkeypatch.setenv("ZRT_POOL", "1" if loop == "pool" else "0")
    img, st = z.render(s, s.camera, p)
    assert same_bits(img, ref)
    for k in COUNTERS:
        assert st[k] == rs[k], k


@pytest.mark.parametrize("loop,hook", [("lockstep", "ZRT_STACK_LDS_ROWS"), ("pool", "ZRT_STACK_LDS_ROWS"),
                                       ("wavefront", "ZRT_STACK_LDS_ROWS16"), ("pool", "ZRT_STACK_LDS_ROWS16")],
                         ids=["lockstep", "pool", "wavefront-rows16", "pool-rows16"])
def test_device_row_bounds_check_reports(scenes, loop, hook, monkeypatch):
    """VERDICT r05 next #4, the device half: the STATS flavour checks every global
    attenuation-row and stack-overflow-row index against its buffer (render.hip
    row_ok, KArgs::att_cap / ovf_cap).  Told the buffers hold nothing
    (ZRT_DEBUG_ROW_CAP=0, honoured by STATS launches only; the real buffers stay
    full size, so nothing is read or written out of bounds either way), a depth-20
    frame whose paths push attenuation rows past the LDS ones and whose traversal
    stack is forced into its global rows (ZRT_STACK_LDS_ROWS=2: a 32-bit stack;
    ZRT_STACK_LDS_ROWS16=2: the 16-bit stack this tree gets, in the wavefront and
    path-pool loops) must fail with
    the bounds error - not fault, not pass; the same launch without the cap passes
    and equals the timed flavour's frame."""
    s = scenes(3)
    p = z.RenderParams(128, 128, 4, 20, flags=z.ZRT_FLAG_STATS)
    monkeypatch.setenv("ZRT_POOL", "1" if loop == "pool" else "0")
    if loop == "wavefront":
        monkeypatch.setenv("ZRT_WF", "1")
    monkeypatch.setenv(hook, "2")
    plan = z.debug_launch_plan(s, p)
    assert plan["stk16"] == (1 if hook == "ZRT_STACK_LDS_ROWS16" else 0) and plan["stack_rows"] == 2
    if hook == "ZRT_STACK_LDS_ROWS16":
        assert plan["sampling_loop"] == {"wavefront": 4, "pool": 5}[loop]
    img, st = z.render(s, s.camera, p)
    ref, _ = z.render(s, s.camera, z.RenderParams(128, 128, 4, 20))
    assert same_bits(img, ref)
    monkeypatch.setenv("ZRT_DEBUG_ROW_CAP", "0")
    with pytest.raises(z.ZrtError, match="past its buffer"):
        z.render(s, s.camera, p)
    z.render(s, s.camera, z.RenderParams(128, 128, 4, 20))  # (the timed flavour ignores the cap)


def _step_eff(s, p):
    """Lane steps / (64 x loop trips that ran one) of a STATS launch (slots 22, 23)."""
    import torch
    ctx = z.RenderContext(s, p)
    buf = torch.zeros(ctx.tile_count(p) * 64 * 3, dtype=torch.float32, device="cuda")
    ctx.render_tiles(s.camera, z.RenderParams(**{**p.__dict__, "flags": z.ZRT_FLAG_STATS}), buf.data_ptr())
    ctx.sync()
    dc = ctx.debug_counters(32)
    ctx.close()
    return dc[23] / (64.0 * dc[22])


@pytest.mark.parametrize("idx,free", [(3, True), (2, False)])
def test_auto_sync_from_probe(scenes, idx, free, monkeypatch):
    """The lockstep interval the render launch takes from the scheduling probe
    (render.hip auto_sync): the teapot (C3's scene), whose waves mostly wait for their
    longest path, runs its lanes free through the unit - more lanes step per loop
    trip - and the bunny (C4's) keeps them in step; either way the frame and the
    counters are the fixed interval's, bit for bit."""
    s = scenes(idx)
    p = z.RenderParams(128, 128, 128, 20)
    monkeypatch.setenv("ZRT_AUTO_SYNC", "0")
    ref, rs = z.render(s, s.camera, p)
    fixed = _step_eff(s, p)
    monkeypatch.delenv("ZRT_AUTO_SYNC")
    img, st = z.render(s, s.camera, p)
    auto = _step_eff(s, p)
    assert same_bits(img, ref)
    for k in COUNTERS:
        assert st[k] == rs[k], k
    if free:
        assert auto > fixed + 0.05, (auto, fixed)
    else:
        assert auto == fixed, (auto, fixed)

"""The temporal step's defaults, what it gains and what it costs; the
sibling of tools/denoise_guided_probe.py.

(a) defaults: for loaded scenes 1 and 2 and the "glass-inside" and "bubbles" scenes of
    tests/shading_scenes.py at 64 x 64, two sequences of 8 frames of 32 spp in chunks of 4
    (seeds seed + k) are rendered once - a static camera, and a truck of TRUCK horizontals
    per frame (zrt-raytrace's ZRT_TEMPORAL_TRUCK rule) - each frame with its variance plane
    and features, with a 4096-spp frame at the last camera.  Every point of the grid
    (alpha_min, max_history, sigma_normal, sigma_depth, without and with ZRT_TA_DEMODULATE)
    runs zrt_ctx_temporal over the 8 frames and the default guided filter on the last
    accumulated frame; its score per sequence is that frame's RMSE over the RMSE of the
    guided filter alone on the last frame, and its score the geometric mean of the 8 ratios
    (they are factors: the arithmetic mean lets the one sequence in which reprojection is not
    valid at all - the truck inside the glass sphere, whose whole frame is refraction - outvote
    the seven others and picks the shortest history of the grid; that winner is recorded too).
    The winner is the lowest score among the points whose static sequences all have a ratio
    below 1 (the condition of tests/test_gpu_temporal.py).  defaults.json, with every point's
    ratios; zrt_temporal_defaults returns the winner (post.cpp ZRT_TA_*).
    quality.json: the winner's ratios per scene and sequence, the parallax of the truck
    (pixels between the first and the last camera, from the last frame's depths), and the
    spread: the sequences rendered again from two other base seeds, (max - min) of each
    sequence's ratio over the three.
(b) bunny: config C4's frame (scene 2, 2048 x 2048, 8 spp in chunks of 4): the device time of
    zrt_ctx_temporal (zrt_ctx_temporal_ms) with a static and with a moving camera at the
    defaults, with a moving camera and everything on (both tests, ZRT_TA_DEMODULATE, a history
    of 32), and of the guided default filter, interleaved, the median of --reps calls each.
    bunny_2048.json.

Each step is a process of its own under `timeout`; a step that fails ends the tool.

usage: python tools/temporal_probe.py --out DIR [--reps 5] [--only defaults|bunny]
       python tools/temporal_probe.py --step defaults|bunny     (one step, JSON on stdout)
"""
import argparse
import dataclasses
import itertools
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from denoise_probe import SCENES, rmse, scene_of, write_json  # noqa: E402

SIZE, SPP, CHUNK, REF_SPP, DEPTH, FRAMES, TRUCK = 64, 32, 4, 4096, 20, 8, 0.03
GRID = {"alpha_min": [0.0, 0.05, 0.1, 0.2, 0.4],
        "max_history": [2, 4, 8, 32],
        "sigma_normal": [0.0, 2.0 ** -4, 2.0 ** -2, 1.0],
        "sigma_depth": [0.0, 2.0 ** -6, 2.0 ** -4, 2.0 ** -2],
        "flags": [0, 1]}
KEYS = list(GRID)
F = np.float32


def truck(T, cam0, k, delta):
    """Frame k's camera: zrt-raytrace's rule, origin and corner plus (float(k) * delta) * horizontal."""
    c = cam0.copy()
    f = F(k) * F(delta)
    c[0] = cam0[0] + f * cam0[2]
    c[1] = cam0[1] + f * cam0[2]
    return T.cam_struct(c)


class Sequence:
    """A scene's frames, variance planes and features on the device, the guided filter alone on
    the last frame and the reference at the last camera."""

    def __init__(self, z, T, key, delta, seed, w=SIZE, h=SIZE, spp=SPP, frames=FRAMES, ref_spp=REF_SPP):
        import torch
        self.key, self.delta = key, delta
        self.keep, view, cam0 = scene_of(z, key)
        cam0 = T.cam_array(cam0)
        self.p = p = z.RenderParams(w, h, spp, DEPTH, sample_chunk=CHUNK, seed=seed)
        self.ctx = ctx = z.RenderContext(view, p)
        n = ctx.tile_count(p)
        tiles = torch.zeros(n * 64 * 3, dtype=torch.float32, device="cuda")
        var_tiles = torch.zeros(n * 64, dtype=torch.float32, device="cuda")
        self.cams = [truck(T, cam0, k, delta) for k in range(frames)]
        self.frames = []
        for k, cam in enumerate(self.cams):
            pk = dataclasses.replace(p, seed=seed + k)
            frame = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
            var = torch.zeros(h * w, dtype=torch.float32, device="cuda")
            feat = torch.zeros(h * w * 8, dtype=torch.float32, device="cuda")
            ctx.accum_begin(cam, pk)
            ctx.accum_pass(spp, tiles.data_ptr())
            ctx.assemble(pk, tiles.data_ptr(), frame.data_ptr())
            ctx.accum_variance(var_tiles.data_ptr())
            ctx.assemble_plane(pk, var_tiles.data_ptr(), var.data_ptr())
            ctx.features(cam, pk, feat.data_ptr())
            ctx.sync()
            torch.cuda.synchronize()
            self.frames.append((frame, feat, var))
        self.acc = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
        self.accv = torch.zeros(h * w, dtype=torch.float32, device="cuda")
        self.out = torch.zeros(h * w * 3, dtype=torch.float32, device="cuda")
        self.dn, self.dn_flags = z.denoise_guided_defaults()
        self.w, self.h = w, h
        if ref_spp:
            self.ref, _ = z.render(view, self.cams[-1],
                                   dataclasses.replace(p, samples_per_pixel=ref_spp, sample_chunk=0))
            frame, feat, var = self.frames[-1]
            self.e_alone = self.filtered(frame, feat, var)
            # the truck's parallax between the first and the last camera, at the last frame's first hits
            f = feat.cpu().numpy().reshape(h, w, 8)[:, :h]
            hit = np.ascontiguousarray(f[..., 7]).view(np.uint32) != 0
            o, llc, H, W = T.cam_array(self.cams[-1])
            x = np.arange(h, dtype=F)[None, :].repeat(h, 0)
            y = np.arange(h, dtype=F)[:, None].repeat(h, 1)
            e = ((llc + H * (x / F(w))[..., None]) + W * (y / F(h))[..., None]) - o
            P = o + e / np.sqrt((e * e).sum(-1))[..., None] * f[..., 3:4]
            plan = T.reproject_plan(T.cam_array(self.cams[0]))
            d = P - plan["origin"]
            with np.errstate(all="ignore"):
                fx = T._dot(d, plan["ru"]) / T._dot(d, plan["rn"]) * F(w)
            shift = np.abs(fx - x)[hit]
            self.parallax = [round(float(shift.mean()), 3), round(float(shift.max()), 3)] if hit.any() else [0.0, 0.0]

    def filtered(self, frame, feat, var):
        import torch
        self.ctx.denoise_guided(self.p, self.dn, self.dn_flags, frame.data_ptr(), feat.data_ptr(), var.data_ptr(),
                                self.out.data_ptr())
        self.ctx.denoise_ms()
        torch.cuda.synchronize()
        return rmse(self.out.cpu().numpy().reshape(self.h, self.w, 3), self.ref, self.h)

    def score(self, tp):
        """RMSE of the last frame after the temporal step over the sequence and the guided filter."""
        self.ctx.temporal_reset()
        for cam, (frame, feat, var) in zip(self.cams, self.frames):
            self.ctx.temporal(cam, self.p, tp, frame.data_ptr(), feat.data_ptr(), var.data_ptr(), self.acc.data_ptr(),
                              self.accv.data_ptr())
        return self.filtered(self.acc, self.frames[-1][1], self.accv)


def step_defaults():
    import temporal_ref as T
    import zraytrace_amd as z
    from zraytrace_amd import _ffi

    def sequences(seed):
        return [Sequence(z, T, key, delta, seed) for key in SCENES for delta in (0.0, TRUCK)]

    data = sequences(42)
    rows = []
    for point in itertools.product(*[GRID[k] for k in KEYS]):
        tp = _ffi.Temporal(**dict(zip(KEYS, point)))
        errs = [d.score(tp) for d in data]
        ratios = [e / d.e_alone for e, d in zip(errs, data)]
        rows.append({"point": list(point), "rmse": [round(e, 6) for e in errs], "ratio": [round(r, 4) for r in ratios],
                     "mean": round(float(np.exp(np.mean(np.log(ratios)))), 5),
                     "arithmetic_mean": round(float(np.mean(ratios)), 5),
                     "static_improves_all": all(r < 1.0 for r, d in zip(ratios, data) if d.delta == 0.0)})
    ok = [r for r in rows if r["static_improves_all"]]
    win = min(ok, key=lambda r: r["mean"])
    marg = {}
    for i, k in enumerate(KEYS):
        marg[k] = []
        for v in GRID[k]:
            sel = [r["mean"] for r in ok if r["point"][i] == v]
            marg[k].append([v, min(sel) if sel else None, len(sel)])
    names = [f"{d.key} {'truck' if d.delta else 'static'}" for d in data]
    defaults = {"step": "defaults", "build_id": z.build_id(), "size": SIZE, "spp": SPP, "sample_chunk": CHUNK,
                "frames": FRAMES, "truck_delta": TRUCK, "reference_spp": REF_SPP, "max_depth": DEPTH,
                "guided_filter": {**data[0].dn.as_dict(), "flags": data[0].dn_flags}, "sequences": names,
                "grid": GRID, "rmse_guided_alone": [round(d.e_alone, 6) for d in data], "points": len(rows),
                "points_improving_every_static_sequence": len(ok),
                "score": "geometric mean over the sequences of rmse(temporal + guided) / rmse(guided alone), last frame",
                "winner_by_arithmetic_mean": (lambda r: {"point": r["point"], "ratio": r["ratio"],
                                                         "arithmetic_mean": r["arithmetic_mean"], "score": r["mean"]})(
                    min(ok, key=lambda r: r["arithmetic_mean"])),
                "rows_columns": KEYS + ["ratio " + n for n in names],
                "rows": [r["point"] + r["ratio"] for r in rows],
                "marginal_columns": ["value", "lowest score among the admissible points", "admissible points"],
                "marginals": marg, "top_columns": KEYS + ["ratio " + n for n in names] + ["score"],
                "top": [r["point"] + r["ratio"] + [r["mean"]] for r in sorted(ok, key=lambda r: r["mean"])[:10]],
                "winner": dict(zip(KEYS, win["point"])), "winner_ratio": win["ratio"], "winner_score": win["mean"]}
    # the winner's ratios from two more base seeds: the spread of the measurement
    tp = _ffi.Temporal(**defaults["winner"])
    ratios = [[e / d.e_alone for e, d in zip(win["rmse"], data)]]
    for seed in (1042, 2042):
        for d in data:
            d.ctx.close()
        data = sequences(seed)
        ratios.append([d.score(tp) / d.e_alone for d in data])
    ratios = np.array(ratios)
    spread = (ratios.max(0) - ratios.min(0))
    first = sequences(42)
    quality = {"what": "tools/temporal_probe.py at zrt_temporal_defaults: 64 x 64, 8 frames of 32 spp in chunks of 4, "
                       "depth 20; RMSE of the last frame against 4096 spp at the last camera, after temporal + guided "
                       "and after the guided filter alone; ratio = the first over the second",
               "truck_delta": TRUCK, "frames": FRAMES, "seeds": [42, 1042, 2042],
               "scenes": {}}
    for i, d in enumerate(first):
        e = d.score(tp)
        quality["scenes"].setdefault(str(d.key), {})["truck" if d.delta else "static"] = {
            "rmse_temporal_guided": round(e, 6), "rmse_guided_alone": round(d.e_alone, 6),
            "ratio": round(e / d.e_alone, 4), "ratio_by_seed": [round(float(r), 4) for r in ratios[:, i]],
            "spread": round(float(spread[i]), 4),
            "parallax_px_mean_max": d.parallax}
    for d in data + first:
        d.ctx.close()
    print(json.dumps({"defaults": defaults, "quality": quality}))


def step_bunny(reps):
    import torch

    import temporal_ref as T
    import zraytrace_amd as z
    w = h = 2048
    d = Sequence(z, T, 2, TRUCK, 42, w, h, 8, 2, 0)
    from zraytrace_amd import _ffi
    tp = z.temporal_defaults()
    full = _ffi.Temporal(alpha_min=0.0, max_history=32, sigma_normal=0.25, sigma_depth=0.0625, flags=1)
    out_len = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    (fa, feat_a, va), (fb, feat_b, vb) = d.frames
    cam_a, cam_b = d.cams

    def temporal(cam, frame, feat, var, tp=tp):
        d.ctx.temporal(cam, d.p, tp, frame.data_ptr(), feat.data_ptr(), var.data_ptr(), d.acc.data_ptr(),
                       d.accv.data_ptr(), out_len.data_ptr())
        return d.ctx.temporal_ms()

    def guided():
        d.ctx.denoise_guided(d.p, d.dn, d.dn_flags, d.acc.data_ptr(), feat_a.data_ptr(), d.accv.data_ptr(),
                             d.out.data_ptr())
        return d.ctx.denoise_ms()

    ms = {"temporal_first_frame": [], "temporal_static": [], "temporal_moving": [], "temporal_moving_everything_on": [],
          "guided": []}
    blended = {}
    for rep in range(reps + 1):  # (the first round is a warm-up)
        d.ctx.temporal_reset()
        t = {"temporal_first_frame": temporal(cam_a, fa, feat_a, va),
             "temporal_static": temporal(cam_a, fa, feat_a, va)}
        blended["static"] = int((out_len > 1).sum().item())
        t["temporal_moving"] = temporal(cam_b, fb, feat_b, vb)
        blended["moving"] = int((out_len > 1).sum().item())
        d.ctx.temporal_reset()  # (a change of ZRT_TA_DEMODULATE drops the history: build one with the flag)
        temporal(cam_a, fa, feat_a, va, full)
        t["temporal_moving_everything_on"] = temporal(cam_b, fb, feat_b, vb, full)
        blended["moving_everything_on"] = int((out_len > 1).sum().item())
        t["guided"] = guided()
        if rep:
            for k, v in t.items():
                ms[k].append(round(v, 4))
    plane = h * h
    out = {"step": "bunny", "build_id": z.build_id(), "width": w, "height": h, "spp": 8, "sample_chunk": 4,
           "max_depth": DEPTH, "reps": reps, "temporal": tp.as_dict(), "temporal_everything_on": full.as_dict(), "truck_delta": TRUCK,
           "pixels_with_history": blended, "ms": ms,
           "ms_median": {k: round(float(np.median(v)), 4) for k, v in ms.items()},
           "bytes_moved_per_frame_minimum": {
               "read": plane * (12 + 4 + 32 + 16 + 16 + 4 + 4), "write": plane * (12 + 4 + 4 + 16 + 32 + 4),
               "note": "per pixel: frame, variance and features in; one history tap (history, first feature float4, "
                       "id word, length) at least; output colour, variance and length, and the next state out"},
           "guided_sigmas": d.dn.as_dict(), "guided_flags": d.dn_flags}
    d.ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=400)
    ap.add_argument("--only")
    a = ap.parse_args()
    if a.step == "defaults":
        return step_defaults()
    if a.step == "bunny":
        return step_bunny(a.reps)
    if not a.out:
        ap.error("--out DIR")
    os.makedirs(a.out, exist_ok=True)
    for name in ("defaults", "bunny"):
        if a.only and a.only != name:
            continue
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:  # nothing more is started on the GPU after a failed step
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(f"step {name} failed with status {r.returncode}")
        d = json.loads(r.stdout.strip().splitlines()[-1])
        if name == "defaults":
            write_json(os.path.join(a.out, "defaults.json"), d["defaults"])
            write_json(os.path.join(a.out, "quality.json"), d["quality"])
            print("winner", d["defaults"]["winner"], d["defaults"]["winner_ratio"], d["defaults"]["winner_score"])
            print("quality", json.dumps(d["quality"]), flush=True)
        else:
            write_json(os.path.join(a.out, "bunny_2048.json"), d)
            print(name, {k: v for k, v in d.items() if k != "ms"}, flush=True)


if __name__ == "__main__":
    main()

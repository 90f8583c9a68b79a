#!/usr/bin/env python
"""What flow visualisation costs on one MI355X, beside the host colouring it replaces (nothing is asserted).

At 8 x 448 x 1024: pwcnet_amd.flow_to_color with and without the max-radius pass, the six-tile pyramid_montage (the frame and
the five pyramid levels of a 448 x 1024 forward), flow_error_color -- device events around chains of calls, median over the
repeats with the extremes -- each beside the bytes it moves at 8 TB/s; the host flow_io.flow_to_color over the same eight fields
(wall clock, one pass per repeat); and infer_continuous.py's seconds per pair with --vis host and --vis gpu on a short synthetic
sequence, un-learned weights, PNG encoding and file writes included (a child process each, its start-up and model build taken
out by subtracting a run over fewer frames).

    python scripts/bench_vis.py [--iters 20] [--repeats 9] [--out profiles/vis_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def events_ms(fn, iters, repeats):
    """Median (and min, max) ms per call of fn over `repeats` groups of `iters` calls, device events around each group."""
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))]


def cli_seconds(vis, frames_dir, count, out):
    t0 = time.perf_counter()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "infer_continuous.py"), "-i",
                          *[os.path.join(frames_dir, f"frame_{i:03d}.png") for i in range(count)], "--vis", vis, "--out", out],
                         capture_output=True, text=True, timeout=900)
    if run.returncode != 0:
        raise SystemExit(run.stderr[-2000:])
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--frames", type=int, default=25, help="frames of the synthetic sequence of the CLI measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import pwcnet_amd
    from pwcnet_amd import flow_io
    torch.cuda.set_device(0)
    N, H, W = 8, 448, 1024
    g = torch.Generator(device="cuda").manual_seed(1)
    flows = torch.randn((N, H, W, 2), device="cuda", generator=g) * 7.0
    gt = flows + torch.randn((N, H, W, 2), device="cuda", generator=g)
    valid = torch.rand((N, H, W), device="cuda", generator=g) < 0.8
    frames = (torch.rand((N, H, W, 3), device="cuda", generator=g) * 255).to(torch.uint8)
    levels = [torch.randn((N, H >> s, W >> s, 2), device="cuda", generator=g) for s in (6, 5, 4, 3, 2)]
    scales = [20.0 / 2 ** (6 - l) for l in range(5)]
    rad = pwcnet_amd.flow_max_radius(flows)
    montage = pwcnet_amd.pyramid_montage(frames, levels, scales)
    torch.cuda.synchronize()
    px = N * H * W
    level_px = sum(int(f.shape[1] * f.shape[2]) * N for f in levels)
    res = {"what": "flow visualisation on the GPU beside the host colouring (context only); medians [min, max]",
           "shape": [N, H, W], "iters": args.iters, "repeats": args.repeats, "hbm_bytes_per_s": HBM_BYTES_PER_S,
           "device": torch.cuda.get_device_name(0)}

    def entry(name, fn, nbytes):
        fn()
        torch.cuda.synchronize()
        ms, span = events_ms(fn, args.iters, args.repeats)
        res[name] = {"ms": ms, "ms_min_max": span, "bytes": nbytes, "ms_at_8TBps": 1e3 * nbytes / HBM_BYTES_PER_S}

    entry("flow_to_color_given_radius", lambda: pwcnet_amd.flow_to_color(flows, rad), px * (8 + 3))
    entry("flow_to_color_own_radius", lambda: pwcnet_amd.flow_to_color(flows), px * (8 + 8 + 3))
    entry("flow_max_radius", lambda: pwcnet_amd.flow_max_radius(flows), px * 8)
    entry("pyramid_montage_six_tiles", lambda: pwcnet_amd.pyramid_montage(frames, levels, scales),
          px * 3 + 2 * level_px * 8 + int(montage.numel()))
    entry("flow_error_color", lambda: pwcnet_amd.flow_error_color(flows, gt, valid), px * (8 + 8 + 1 + 3))
    res["pyramid_montage_six_tiles"]["out_shape"] = list(montage.shape)

    host = flows.cpu().numpy()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        for n in range(N):
            flow_io.flow_to_color(host[n])
        ts.append((time.perf_counter() - t0) * 1e3)
    res["host_flow_to_color_8_fields"] = {"ms": float(np.median(ts)), "ms_min_max": [float(min(ts)), float(max(ts))],
                                          "threads": torch.get_num_threads()}
    t0 = time.perf_counter()
    flows.cpu()
    torch.cuda.synchronize()
    res["copy_back_float32_8_fields_ms"] = (time.perf_counter() - t0) * 1e3

    # the sequence CLI: seconds per pair, PNG encoding included; (long run - short run) / (pairs more) takes the start-up out
    from PIL import Image
    rng = np.random.RandomState(3)
    base = rng.uniform(0, 255, size=(448, 1024, 3)).astype(np.uint8)
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(args.frames):
            Image.fromarray(np.roll(base, 3 * i, axis=1)).save(os.path.join(tmp, f"frame_{i:03d}.png"))
        short = 2
        cli = {}
        for vis in ("host", "gpu"):
            t_short = cli_seconds(vis, tmp, short, os.path.join(tmp, "out_" + vis + "_s"))
            t_long = cli_seconds(vis, tmp, args.frames, os.path.join(tmp, "out_" + vis))
            cli[vis] = {"seconds_short_run": t_short, "seconds_long_run": t_long, "pairs_short": short - 1,
                        "pairs_long": args.frames - 1, "seconds_per_pair": (t_long - t_short) / (args.frames - short)}
        picture = np.asarray(Image.open(os.path.join(tmp, "out_gpu", os.path.basename(tmp), "frame_000.png")))
        t0 = time.perf_counter()
        for _ in range(5):
            Image.fromarray(picture).save(os.path.join(tmp, "encode.png"))
        cli["png_encode_seconds_per_montage"] = (time.perf_counter() - t0) / 5
        cli["montage_shape"] = list(picture.shape)
    res["infer_continuous_448x1024"] = cli

    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

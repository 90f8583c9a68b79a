#!/usr/bin/env python
"""Time the cost-volume feature normalisation (PWCDCNet(normalize_features=True), DESIGN.md "Feature normalisation") against
the flag off, which is the path the parent commit runs:

  forward   PWCDCNet at 8 x 448 x 1024, one stream, launch-plan replays between device events, median of the repeats;
  step      Trainer.step at 4 x 384 x 448 (supervised multiscale step, forward + backward + Adam), host clock around
            synchronised groups of steps, median of the repeats; the flag-off run is timed twice, around the other, so that the
            spread of one configuration is on record next to the difference;
  op        the op alone at the five level shapes of the 8 x 448 x 1024 forward, device events around chains of calls.

Expectation: the five levels hold 2 x 52 MB of features (8 pairs, 448 x 1024: 7 x 16 x 192 ... 112 x 256 x 32); they are read
twice and written once, about 0.3 GB, some tens of us at HBM speed (most of it stays in the 256 MB last-level cache), plus ten
launches (two per level): a few percent of a 2.3 - 2.6 ms forward.  Nothing is asserted.  Prints one JSON
line and writes it to --out.

    python scripts/bench_featnorm.py [--iters 30] [--repeats 9] [--steps 10] [--no-step] [--out profiles/featnorm_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
LEVEL_CHANNELS = (192, 128, 96, 64, 32)


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


def forward_times(iters, repeats):
    import pwcnet_amd
    from tests import util
    N, H, W = 8, 448, 1024
    w = util.model_weights(False)
    im0, im1 = (torch.from_numpy(a).cuda() for a in util.smooth_images(N, H, W))
    res = {"shape": [N, H, W]}
    nets = {}
    for key, flag in (("off", False), ("on", True)):
        nets[key] = pwcnet_amd.PWCDCNet(normalize_features=flag, range_check="off")
        nets[key].load_weights(w)
        for _ in range(3):
            nets[key](im0, im1)
    torch.cuda.synchronize()
    for key in ("off", "on", "off_again"):
        net = nets[key.split("_")[0]]
        res[f"forward_ms_{key}"], res[f"forward_ms_{key}_min_max"] = events_ms(lambda: net(im0, im1), iters, repeats)
    res["forward_ms_on_minus_off"] = res["forward_ms_on"] - 0.5 * (res["forward_ms_off"] + res["forward_ms_off_again"])
    return res


def op_times(iters, repeats):
    from pwcnet_amd.modules import FeatureNormLayer, View
    N, H, W = 8, 448, 1024
    layer = FeatureNormLayer()
    res, total_us, total_bytes = {}, 0.0, 0
    for l, C in enumerate(LEVEL_CHANNELS):
        h, w = H >> (6 - l), W >> (6 - l)
        x = torch.randn((2 * N, h, w, C), device="cuda")
        y = torch.empty_like(x)
        stats = torch.empty((N, 2), dtype=torch.float64, device="cuda")
        ws = layer.workspace(N, h, w, C, "cuda")
        half = 4 * N * h * w * C
        views = [View(t.data_ptr() + o, C, N, h, w, C) for t in (x, y) for o in (0, half)]
        ms, mm = events_ms(lambda: layer._run(views[0], views[1], views[2], views[3], stats, ws), iters, repeats)
        nbytes = 3 * x.numel() * 4                                  # read twice, written once
        res[f"{h}x{w}x{C}"] = {"us": 1e3 * ms, "us_min_max": [1e3 * t for t in mm], "bytes": nbytes,
                               "us_at_8TBps": 1e6 * nbytes / HBM_BYTES_PER_S}
        total_us += 1e3 * ms
        total_bytes += nbytes
    res["sum_us"], res["sum_bytes"] = total_us, total_bytes
    return res


def step_times(steps, repeats):
    from pwcnet_amd.train import Trainer
    from tests import util
    N, H, W = 4, 384, 448
    im0, im1 = (torch.from_numpy(a).cuda() for a in util.smooth_images(N, H, W))
    gt = torch.from_numpy(util.flow_field(N, H, W, outliers=False).astype(np.float32)).cuda()
    res = {"shape": [N, H, W]}
    tns = {}
    for key, flag in (("off", False), ("on", True)):
        tns[key] = Trainer(lr=1e-6, normalize_features=flag)
        for _ in range(3):
            tns[key].step(im0, im1, gt)
    for key in ("off", "on", "off_again"):
        tn = tns[key.split("_")[0]]
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tn.step(im0, im1, gt)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0) / steps)
        res[f"step_ms_{key}"], res[f"step_ms_{key}_min_max"] = float(np.median(ts)), [float(min(ts)), float(max(ts))]
    res["step_ms_on_minus_off"] = res["step_ms_on"] - 0.5 * (res["step_ms_off"] + res["step_ms_off_again"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="skip the training step timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_featnorm.py needs a GPU")
    res = {"what": "PWCDCNet / Trainer with normalize_features on against off (the parent's path); one stream, medians",
           "command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:]),
           "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "forward": forward_times(args.iters, args.repeats), "op": op_times(args.iters, args.repeats)}
    if not args.no_step:
        res["step"] = step_times(args.steps, args.repeats)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

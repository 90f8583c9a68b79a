#!/usr/bin/env python
"""Time the batch preparation of train.py at Sintel's size, both ways, for one batch of 8 pairs of 436 x 1024 frames cut to
384 x 448:

  --augment full   pwcnet_amd.augment_pairs on uint8 frames, flow and mask already on the GPU: device events around one call
                   (the upload of the records included), median of --runs after warm-up; beside it the host's share of the
                   step (draw_params) and the upload of the whole uint8 frames, flow and mask, by the host clock around a
                   device synchronise.
  --augment none   what train.py does for the same batch today: the host crop of float32 frames, np.stack, / 255, and the
                   float32 upload of frames, flow and mask; host clock around a device synchronise, median of --runs.

No time is a pass / fail condition.  Prints plain lines (profiles/augment_gpu_test_figures.txt keeps them).

    python scripts/bench_augment.py [--batch 8] [--size 436 1024] [--crop 384 448] [--runs 50]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_ms(fn, runs, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", nargs=2, type=int, default=[436, 1024], metavar=("H", "W"))
    ap.add_argument("--crop", nargs=2, type=int, default=[384, 448], metavar=("OH", "OW"))
    ap.add_argument("--runs", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py needs a GPU")
    from pwcnet_amd import augment_pairs, draw_params
    B, (H, W), crop = args.batch, args.size, tuple(args.crop)
    rs = np.random.RandomState(0)
    im0 = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    im1 = rs.randint(0, 256, size=(B, H, W, 3)).astype(np.uint8)
    flow = rs.normal(0, 3, size=(B, H, W, 2)).astype(np.float32)
    valid = rs.uniform(size=(B, H, W)) >= 0.05
    full = dict(scale=(0.9, 1.3), rotate_deg=10.0, translate_frac=0.1, flip=0.5, rel_rotate_deg=1.0, rel_translate_px=2.0, color=True)
    rng = np.random.RandomState(1)
    d0, d1, df, dv = (torch.from_numpy(a).cuda() for a in (im0, im1, flow, valid))
    params = [draw_params(B, (H, W), crop, rng, **full) for _ in range(args.runs + 5)]

    for k in range(5):                                                       # warm-up
        augment_pairs(d0, d1, params[k], crop, flows=df, valid=dv)
    ts = []
    for k in range(args.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        augment_pairs(d0, d1, params[5 + k], crop, flows=df, valid=dv)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    print(f"# python scripts/bench_augment.py --batch {B} --size {H} {W} --crop {crop[0]} {crop[1]} --runs {args.runs}   "
          f"({torch.cuda.get_device_name(0)})")
    print(f"augment_pairs, batch {B}, uint8 {H}x{W} -> {crop[0]}x{crop[1]}, full augmentation, flow and mask: "
          f"{np.median(ts):.3f} ms (device events, median of {args.runs}; min {min(ts):.3f}, max {max(ts):.3f})")
    t = time.perf_counter()
    for _ in range(args.runs):
        draw_params(B, (H, W), crop, rng, **full)
    print(f"draw_params on the host for that batch: {(time.perf_counter() - t) * 1e3 / args.runs:.3f} ms (mean of {args.runs})")
    up = host_ms(lambda: [torch.from_numpy(a).cuda() for a in (im0, im1, flow, valid)], args.runs)
    print(f"upload of the whole uint8 frames, flow and mask ({(im0.nbytes * 2 + flow.nbytes + valid.nbytes) / 1e6:.1f} MB, pageable): "
          f"{up[0]:.3f} ms (host clock, median of {args.runs}; min {up[1]:.3f}, max {up[2]:.3f})")

    # the parent's path: FilePairs.__getitem__'s crop of float32 frames, batches()'s stack, the step's / 255 and uploads
    f0, f1 = im0.astype(np.float32), im1.astype(np.float32)
    crng = np.random.RandomState(2)

    def parent():
        items = []
        for n in range(B):
            y0, x0 = crng.randint(0, H - crop[0] + 1), crng.randint(0, W - crop[1] + 1)
            sl = (slice(y0, y0 + crop[0]), slice(x0, x0 + crop[1]))
            items.append((np.ascontiguousarray(f0[n][sl]), np.ascontiguousarray(f1[n][sl]), np.ascontiguousarray(flow[n][sl]),
                          np.ascontiguousarray(valid[n][sl])))
        a, b, f, v = (torch.from_numpy(np.stack([it[k] for it in items])) for k in range(4))
        return (a / 255.0).cuda(), (b / 255.0).cuda(), f.cuda(), v.cuda()

    pt = host_ms(parent, args.runs)
    print(f"the host path for the same batch (crop, stack, / 255, float32 upload of frames, flow and mask): "
          f"{pt[0]:.3f} ms (host clock, median of {args.runs}; min {pt[1]:.3f}, max {pt[2]:.3f})")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Workload for one `rocprofv3 --kernel-trace --stats` run: fb_valid (csrc/pwc_fbcheck.hip, both directions, with counts) and,
as the yardstick, photometric_sums (photometric_partial_kernel: the same pixel walk, similar traffic) at batch 8 x 448 x 1024,
`--reps` launches each after a warm-up.  Seeded inputs: a shift of up to 4 px per image plus 0.2 px of per-pixel noise as the
forward flow, its negative plus 1.2 px of noise as the backward flow, so that roughly half of the pixels pass the check.

    rocprofv3 --kernel-trace --stats -d <dir> -o fb -- python scripts/profile_fbcheck.py
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--shape", nargs=2, type=int, default=[448, 1024])
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from pwcnet_amd import unsup
    N, (H, W) = args.batch, args.shape
    g = torch.Generator(device="cuda").manual_seed(0)
    fw = torch.empty((N, 1, 1, 2), device="cuda").uniform_(-4.0, 4.0, generator=g) + \
        torch.empty((N, H, W, 2), device="cuda").uniform_(-0.2, 0.2, generator=g)
    bw = -fw + torch.empty((N, H, W, 2), device="cuda").uniform_(-1.2, 1.2, generator=g)
    im0 = torch.empty((N, H, W, 3), device="cuda").uniform_(0.0, 1.0, generator=g)
    im1 = torch.empty((N, H, W, 3), device="cuda").uniform_(0.0, 1.0, generator=g)
    for reps in (3, args.reps):
        for _ in range(reps):
            masks = unsup.fb_valid(fw, bw, return_counts=True)
            sums = unsup.photometric_sums(im0, im1, fw)
        torch.cuda.synchronize()
    print(f"batch {N} x {H} x {W}: valid share fw {float(masks[2].sum()) / (N * H * W):.3f} bw {float(masks[3].sum()) / (N * H * W):.3f}, "
          f"photometric contributing {int(sums[1].sum())} of {N * H * W}")


if __name__ == "__main__":
    main()

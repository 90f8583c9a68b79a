#!/usr/bin/env python
"""Time the temporal filter (pwcnet_amd.temporal_filter) on a clip of 16 frames of 448 x 1024 uint8 RGB for
R in {1, 2, 4} and P in {0, 1}, beside a torch restatement built from grid_sample steps on the same device, which is the route
the op replaces: device events around chains of calls, median of the repeats.

What a call cannot avoid moving: the frames in (T H W 3 bytes), both flows in (2 (T - 1) H W 8 bytes) and the outputs out
(T H W (3 + 1) bytes) -- 161.5 MB at this shape, 20 us at 8 TB/s, whatever R and P are.  The script reports that figure and the
fraction of HBM bandwidth it implies for the measured time.  No speed figure was set in advance: nobody had measured this op.  It
will not come near the bandwidth bound: per neighbour a lane gathers 4 (with the check 8) flow records and (2P+2)^2 pixels of 3
bytes at a position of its own, in a dependent chain of up to R steps per direction, and the arithmetic is in double -- the
gathers are served by the caches (each frame is read by 2 R + 1 output frames), and their latency and the double-precision
rate decide the time.
The grid_sample route is there for context only: float32, the frames as float NCHW, one warp of the whole neighbour frame per
step and an average pool for the patch distance (the patch around p against the warped frame, not the kernel's patch around q),
no masks and no sentinel rule, several full-size intermediates per neighbour.  Nothing is asserted.  Prints one JSON line and
writes it to --out.

    python scripts/bench_temporal.py [--iters 10] [--repeats 7] [--out profiles/temporal_bench.json]
"""
import argparse
import json
import os
import sys

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


def _sample(nchw, x, y, H, W):
    """(1,C,H,W) sampled bilinearly at the (H,W) positions (x, y) by grid_sample (align_corners=True, border)."""
    grid = torch.stack([x * (2.0 / (W - 1)) - 1.0, y * (2.0 / (H - 1)) - 1.0], dim=-1)[None]
    return torch.nn.functional.grid_sample(nchw, grid, mode="bilinear", padding_mode="border", align_corners=True)


def grid_sample_filter(frames_nchw, fw_nchw, bw_nchw, radius, sigma, patch, alpha1=0.01, alpha2=0.5):
    """(filtered (T,3,H,W) float32 grey levels, support (T,H,W)): temporal_filter restated in float32 on grid_sample."""
    T, C, H, W = frames_nchw.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=frames_nchw.device, dtype=torch.float32),
                            torch.arange(W, device=frames_nchw.device, dtype=torch.float32), indexing="ij")
    outs, sups = [], []
    for i in range(T):
        own = frames_nchw[i:i + 1]
        acc, wsum, sup = own.clone(), torch.ones((1, 1, H, W), device=own.device), torch.zeros((H, W), device=own.device)
        for s in (1, -1):
            x, y, alive = xs, ys, torch.ones((H, W), dtype=torch.bool, device=own.device)
            for k in range(1, radius + 1):
                f = i + s * k
                if f < 0 or f >= T:
                    break
                j = i + k - 1 if s > 0 else i - k
                F, G = (fw_nchw, bw_nchw) if s > 0 else (bw_nchw, fw_nchw)
                S = _sample(F[j:j + 1], x, y, H, W)[0]
                rx, ry = x + S[0], y + S[1]
                b = _sample(G[j:j + 1], rx, ry, H, W)[0]
                fine = alpha1 * ((S * S).sum(0) + (b * b).sum(0)) + alpha2 - ((S + b) ** 2).sum(0) >= 0
                alive = alive & (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1) & fine
                x, y = rx, ry
                warped = _sample(frames_nchw[f:f + 1], x, y, H, W)
                d2 = ((own - warped) ** 2).mean(dim=1, keepdim=True)
                if patch > 0:
                    d2 = torch.nn.functional.avg_pool2d(d2, 2 * patch + 1, stride=1, padding=patch, count_include_pad=False)
                w = alive[None, None] / (1.0 + d2 / (sigma * sigma))
                acc, wsum, sup = acc + w * warped, wsum + w, sup + alive
        outs.append(acc / wsum)
        sups.append(sup)
    return torch.cat(outs), torch.stack(sups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_temporal.py needs a GPU")
    import pwcnet_amd as P
    T, H, W, C = 16, 448, 1024, 3
    gen = torch.Generator(device="cuda").manual_seed(0)
    # a smooth picture drifting along a smooth field of a few pixels per step, plus noise; the backward flow is the negative of
    # the forward one: consistent but where the field bends
    coarse = 3.0 * torch.randn((T - 1, 2, 8, 16), device="cuda", generator=gen)
    fw = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous()
    bw = (-fw).contiguous()
    picture = torch.nn.functional.interpolate(torch.rand((1, C, 28, 64), device="cuda", generator=gen), size=(H, W), mode="bilinear",
                                              align_corners=True)
    frames = (255.0 * picture + 10.0 * torch.randn((T, C, H, W), device="cuda", generator=gen)).clamp(0, 255).round()
    frames_u8 = frames.permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    fw_nchw, bw_nchw = fw.permute(0, 3, 1, 2).contiguous(), bw.permute(0, 3, 1, 2).contiguous()
    moved = T * H * W * C + 2 * (T - 1) * H * W * 8 + T * H * W * (C + 1)
    res = {"what": "temporal_filter beside a torch grid_sample restatement (context only); medians of device-event groups",
           "command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:]),
           "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "shape": [T, H, W, C], "dtype": "uint8",
           "sigma": 10.0, "fb_check": True, "bytes_unavoidable": moved, "us_at_8TBps": 1e6 * moved / HBM_BYTES_PER_S, "configs": {}}
    for radius in (1, 2, 4):
        for patch in (0, 1):
            fn = lambda: P.temporal_filter(frames_u8, fw, bw, radius=radius, patch=patch, sigma=10.0)      # noqa: E731
            filtered, support = fn()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms, mm = events_ms(fn, args.iters, args.repeats)
            ref = lambda: grid_sample_filter(frames, fw_nchw, bw_nchw, radius, 10.0, patch)                # noqa: E731
            want, want_sup = ref()
            torch.cuda.synchronize()
            ref_ms, ref_mm = events_ms(ref, max(1, args.iters // 5), min(args.repeats, 3))
            diff = (filtered.permute(0, 3, 1, 2).float() - want).abs()
            res["configs"][f"R{radius}_P{patch}"] = {
                "ms": ms, "ms_min_max": mm, "hbm_fraction_of_8TBps": (moved / (ms * 1e-3)) / HBM_BYTES_PER_S,
                "mean_support": float(support.float().mean()), "grid_sample_ms": ref_ms, "grid_sample_ms_min_max": ref_mm,
                "grid_sample_mean_abs_difference_grey_levels": float(diff.mean()),
                "grid_sample_support_agreement": float((support.float() == want_sup).float().mean())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

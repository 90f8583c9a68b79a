#!/usr/bin/env python
"""Time the background plate (pwcnet_amd.background_plate, plate_difference) on a synthetic pan: frames of
448 x 1024 RGB onto a 512 x 1280 canvas, median and mean at T = 8, 32, 64 for uint8, T = 32 for float32, and plate_difference of
32 frames, beside a torch restatement on the same device, which is the route the op replaces: device events around chains of
calls, median of the repeats.

What a build cannot avoid moving: the frames in once (T H W C elements) and plate and count out (Hc Wc (C elements + 1 byte)).
The script reports that figure, the time it takes at 8 TB/s and the fraction of that rate the measured time implies.  The figure
IGNORES RE-READS: a canvas pixel gathers four corners per frame, neighbouring lanes share them through the caches, and a float
plate gathers the corners of channels 1 .. C - 1 a second time; the median's 8 (bytes) or 32 C (floats) selection rounds over
the T slots run in the LDS and move nothing.  No speed figure was set in advance: nobody had measured this op.
The torch route is there for context only: float32, grid_sample of every frame onto the canvas (align_corners=True, zeros
outside) into a (T, Hc, Wc, C) stack with NaN where a frame does not cover the canvas, then torch.nanmedian / nanmean over the
frames.  nanmedian also takes the lower of two middle values; its samples are float32 blends, not rounded bytes, so the bytes may
differ by one grey level.  Nothing is asserted.  Prints one JSON line and writes it to --out.

    python scripts/bench_plate.py [--iters 10] [--repeats 7] [--out profiles/plate_bench.json]
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


def torch_plate(frames_nchw, matrices, Hc, Wc, mode):
    """(plate (Hc,Wc,C) float32, count (Hc,Wc)): background_plate restated on grid_sample and nanmedian / nanmean."""
    T, C, H, W = frames_nchw.shape
    ys, xs = torch.meshgrid(torch.arange(Hc, device=frames_nchw.device, dtype=torch.float32),
                            torch.arange(Wc, device=frames_nchw.device, dtype=torch.float32), indexing="ij")
    m = matrices.to(torch.float32)
    sx = m[:, 0, 0, None, None] * xs + m[:, 0, 1, None, None] * ys + m[:, 0, 2, None, None]
    sy = m[:, 1, 0, None, None] * xs + m[:, 1, 1, None, None] * ys + m[:, 1, 2, None, None]
    inside = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
    grid = torch.stack([sx * (2.0 / (W - 1)) - 1.0, sy * (2.0 / (H - 1)) - 1.0], dim=-1)
    stack = torch.nn.functional.grid_sample(frames_nchw, grid, mode="bilinear", padding_mode="border", align_corners=True)
    stack = torch.where(inside[:, None], stack, torch.full_like(stack, float("nan")))
    plate = torch.nanmedian(stack, dim=0).values if mode == "median" else torch.nanmean(stack, dim=0)
    return torch.nan_to_num(plate, nan=0.0).permute(1, 2, 0), inside.sum(dim=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plate.py needs a GPU")
    import pwcnet_amd as P
    H, W, C, Hc, Wc, Tmax = 448, 1024, 3, 512, 1280, 64
    gen = torch.Generator(device="cuda").manual_seed(0)
    # one wide smooth scene, every frame a window of it that pans 4 px per frame and bobs a little, plus noise and a moving block
    scene = torch.nn.functional.interpolate(torch.rand((1, C, 32, 80), device="cuda", generator=gen), size=(Hc, Wc), mode="bilinear",
                                            align_corners=True)[0]
    frames, to_frame = [], np.tile(np.eye(3), (Tmax, 1, 1))
    for t in range(Tmax):
        ox, oy = 4 * t, 32 + int(round(20 * np.sin(t / 5.0)))              # the frame's corner on the canvas
        f = 255.0 * scene[:, oy:oy + H, ox:ox + W] + 6.0 * torch.randn((C, H, W), device="cuda", generator=gen)
        f[:, 100:164, (37 * t) % (W - 64):(37 * t) % (W - 64) + 64] = 255.0
        frames.append(f.clamp(0, 255).round())
        ang = np.deg2rad(0.2 * np.sin(t))                                  # a little rotation: the samples are real blends
        to_frame[t] = [[np.cos(ang), -np.sin(ang), -ox + 0.25], [np.sin(ang), np.cos(ang), -oy + 0.5], [0.0, 0.0, 1.0]]
    frames = torch.stack(frames)                                           # (T,C,H,W) float32 grey levels
    frames_u8 = frames.permute(0, 2, 3, 1).contiguous().to(torch.uint8)
    frames_f32 = (frames.permute(0, 2, 3, 1) / 255.0).contiguous()
    matrices = torch.from_numpy(to_frame).cuda()
    back = torch.from_numpy(np.stack([np.linalg.inv(m) for m in to_frame])).cuda()
    back[:, 2] = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device="cuda")
    res = {"what": "background_plate / plate_difference beside a torch grid_sample + nanmedian / nanmean restatement (context only); "
                   "medians of device-event groups; the roofline bytes are the frames read once plus plate and count written and "
                   "ignore re-reads",
           "command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:]),
           "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "frame": [H, W, C], "canvas": [Hc, Wc],
           "configs": {}}
    for dtype, T, mode in [("uint8", T, mode) for T in (8, 32, 64) for mode in ("median", "mean")] + [("float32", 32, "median"),
                                                                                                  ("float32", 32, "mean")]:
        clip = frames_u8[:T] if dtype == "uint8" else frames_f32[:T]
        size = 1 if dtype == "uint8" else 4
        fn = lambda: P.background_plate(clip, matrices[:T], (Hc, Wc), mode=mode)                       # noqa: E731
        plate, count = fn()
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms, mm = events_ms(fn, args.iters, args.repeats)
        ref = lambda: torch_plate(frames[:T], matrices[:T], Hc, Wc, mode)                              # noqa: E731
        want, want_count = ref()
        torch.cuda.synchronize()
        ref_ms, ref_mm = events_ms(ref, max(1, args.iters // 5), min(args.repeats, 3))
        got = plate.float() * (1.0 if dtype == "uint8" else 255.0)
        moved = T * H * W * C * size + Hc * Wc * (C * size + 1)
        res["configs"][f"{dtype}_T{T}_{mode}"] = {
            "ms": ms, "ms_min_max": mm, "bytes_roofline": moved, "us_at_8TBps": 1e6 * moved / HBM_BYTES_PER_S,
            "hbm_fraction_of_8TBps": (moved / (ms * 1e-3)) / HBM_BYTES_PER_S, "mean_count": float(count.float().mean()),
            "torch_ms": ref_ms, "torch_ms_min_max": ref_mm, "torch_over_hip": ref_ms / ms,
            "torch_mean_abs_difference_grey_levels": float((got - want).abs().mean()),
            "torch_count_agreement": float((count.long() == want_count).float().mean())}
        del want, want_count
    T = 32
    plate, count = P.background_plate(frames_u8[:T], matrices[:T], (Hc, Wc))
    fn = lambda: P.plate_difference(frames_u8[:T], plate, count, back[:T], 10.0)                       # noqa: E731
    difference, foreground, known = fn()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms, mm = events_ms(fn, args.iters, args.repeats)
    moved = T * H * W * C + Hc * Wc * (C + 1) + T * H * W * 6              # frames, plate and count in; a float and two bytes out
    res["configs"][f"uint8_T{T}_difference"] = {
        "ms": ms, "ms_min_max": mm, "bytes_roofline": moved, "us_at_8TBps": 1e6 * moved / HBM_BYTES_PER_S,
        "hbm_fraction_of_8TBps": (moved / (ms * 1e-3)) / HBM_BYTES_PER_S, "known_fraction": float(known.float().mean()),
        "foreground_fraction": float(foreground.float().mean())}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

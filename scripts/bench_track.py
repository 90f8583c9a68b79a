#!/usr/bin/env python
"""Time point tracking (pwcnet_amd.track_points) for the grid:4 queries of a 448 x 1024 sequence of T = 16 flows,
with and without the forward-backward check, beside a torch restatement on grid_sample in a Python loop over T, which is the
route the op replaces: device events around chains of calls, median of the repeats.

Expectation, in bytes (written before the first run; nobody had measured this op): P = 112 x 256 = 28672 points.  A step loads
four 8-byte flow records (32 bytes; the two corners of a row are neighbours, so two 16-byte pieces in two rows) and, with the
check, four more of the backward flow, and stores 8 + 1 bytes of track and status: 41 bytes per point and step without the
check, 73 with it -- 18.8 MB and 33.5 MB per call, 2.4 us and 4.2 us at 8 TB/s.  The op cannot come near that: the points of a
stride-4 grid share no cache line along x beyond 16 points, so the traffic is lines (up to 2 per sample), and above all the 16
steps of a point are a dependent chain of gathers (position -> corners -> position -> check corners) carried by only 448 waves,
fewer than two per compute unit.  Latency times T decides the time, not bandwidth; no figure is claimed in advance.
The grid_sample route is there for context only: it permutes the flows to NCHW, launches several kernels per step, has no
status, no masks and no sentinel rule.  Nothing is asserted.  Prints one JSON line and writes it to --out.

    python scripts/bench_track.py [--iters 20] [--repeats 9] [--out profiles/track_bench.json]
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


def _sample(field_nchw, pts, H, W):
    """(P,2): an (1,2,H,W) flow sampled bilinearly at the (P,2) points (x, y) by grid_sample (align_corners=True, border)."""
    grid = torch.stack([pts[:, 0] * (2.0 / (W - 1)) - 1.0, pts[:, 1] * (2.0 / (H - 1)) - 1.0], dim=-1)[None, None]
    return torch.nn.functional.grid_sample(field_nchw, grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0].t()


def grid_sample_track(flows_fw, points, flows_bw=None, alpha1=0.01, alpha2=0.5):
    """(tracks (T+1,P,2), consistent (T,P) or None): the positions of track_points while a point is VISIBLE, to float32 rounding,
    and the forward-backward test per step; no status, nothing stops."""
    T, H, W, _ = flows_fw.shape
    fw = flows_fw.permute(0, 3, 1, 2)
    bw = None if flows_bw is None else flows_bw.permute(0, 3, 1, 2)
    tracks, ok = [points], []
    for t in range(T):
        s = _sample(fw[t:t + 1], tracks[-1], H, W)
        nxt = tracks[-1] + s
        if bw is not None:
            b = _sample(bw[t:t + 1], nxt, H, W)
            ok.append(alpha1 * ((s * s).sum(1) + (b * b).sum(1)) + alpha2 - ((s + b) ** 2).sum(1) >= 0)
        tracks.append(nxt)
    return torch.stack(tracks), (torch.stack(ok) if ok else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_track.py needs a GPU")
    import pwcnet_amd as P
    from pwcnet_amd import track as TK
    T, H, W, stride = 16, 448, 1024, 4
    gen = torch.Generator(device="cuda").manual_seed(0)
    # a smooth field of a few pixels per step, the backward flow its negative: consistent but where the field bends
    coarse = 3.0 * torch.randn((T, 2, 8, 16), device="cuda", generator=gen)
    fw = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).contiguous()
    bw = (-fw).contiguous()
    points = P.grid_points(H, W, stride).cuda()
    n = points.shape[0]
    res = {"what": "track_points beside a torch grid_sample loop over T (context only); medians",
           "command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:]),
           "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "shape": [T, H, W], "points": n,
           "bytes_no_check": 41 * n * T, "bytes_check": 73 * n * T,
           "us_at_8TBps_no_check": 1e6 * 41 * n * T / HBM_BYTES_PER_S, "us_at_8TBps_check": 1e6 * 73 * n * T / HBM_BYTES_PER_S}
    for key, kw in (("no_check", {}), ("check", dict(flows_bw=bw)), ("check_keep_stepping", dict(flows_bw=bw, stop_on_occlusion=False))):
        fn = lambda: P.track_points(fw, points, **kw)                          # noqa: E731
        _, status = fn()
        res[f"last_slice_{key}"] = {name: int((status[-1] == c).sum()) for c, name in enumerate(TK.STATUS_NAMES)}
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms, mm = events_ms(fn, args.iters, args.repeats)
        res[f"track_{key}"] = {"us": 1e3 * ms, "us_min_max": [1e3 * t for t in mm]}
    tracks, status = P.track_points(fw, points)
    seen = (status == TK.VISIBLE).all(dim=0)
    ref, _ = grid_sample_track(fw, points)
    res["grid_sample_max_abs_difference_where_visible"] = float((ref - tracks)[:, seen].abs().max()) if bool(seen.any()) else None
    for key, kw in (("no_check", {}), ("check", dict(flows_bw=bw))):
        fn = lambda: grid_sample_track(fw, points, **kw)                       # noqa: E731
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms, mm = events_ms(fn, args.iters, args.repeats)
        res[f"grid_sample_{key}"] = {"us": 1e3 * ms, "us_min_max": [1e3 * t for t in mm]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

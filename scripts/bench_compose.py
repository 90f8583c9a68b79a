#!/usr/bin/env python
"""Time flow composition (pwcnet_amd.compose_flows / compose_grad, DESIGN.md "Flow composition") at 8 x 448 x 1024 beside a torch
restatement of the same thing on grid_sample, which is the route the op replaces: device events around chains of calls, median
of the repeats, with and without both masks.

Expectation: the forward reads 8 bytes of flow_ab per pixel, gathers flow_bc (8 bytes per pixel where neighbours share their
corners through the caches), and writes 8 + 1 bytes: about 25 bytes per pixel, 92 MB, some 12 us at 8 TB/s -- so launch latency
and the gather through L2 decide its time, not HBM.  The gradient zeroes and re-reads 16 bytes of accumulators per pixel, runs the
sample twice (per-image maximum, scatter) and adds eight 64-bit atomics per valid pixel: the atomics decide it.
The grid_sample route is there for context only: it permutes to NCHW, has no validity and no sentinel rule, and its backward adds
floats with atomics (its bits change from call to call).  Nothing is asserted.  Prints one JSON line and writes it to --out.

    python scripts/bench_compose.py [--iters 20] [--repeats 9] [--out profiles/compose_bench.json]
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


def grid_sample_compose(ab, bc):
    """flows_ac = ab + bc sampled at p + ab, by torch.nn.functional.grid_sample (align_corners=True, border padding): the values
    of compose_flows at its valid pixels, to float32 rounding; no mask, no sentinel."""
    N, H, W, _ = ab.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=ab.device, dtype=torch.float32),
                            torch.arange(W, device=ab.device, dtype=torch.float32), indexing="ij")
    gx = (xs[None] + ab[..., 0]) * (2.0 / max(W - 1, 1)) - 1.0
    gy = (ys[None] + ab[..., 1]) * (2.0 / max(H - 1, 1)) - 1.0
    sampled = torch.nn.functional.grid_sample(bc.permute(0, 3, 1, 2), torch.stack([gx, gy], dim=-1), mode="bilinear",
                                              padding_mode="border", align_corners=True)
    return ab + sampled.permute(0, 2, 3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compose.py needs a GPU")
    import pwcnet_amd as P
    N, H, W = 8, 448, 1024
    gen = torch.Generator(device="cuda").manual_seed(0)
    ab = 4.0 * torch.randn((N, H, W, 2), device="cuda", generator=gen)
    bc = 4.0 * torch.randn((N, H, W, 2), device="cuda", generator=gen)
    va = torch.rand((N, H, W), device="cuda", generator=gen) < 0.9
    vb = torch.rand((N, H, W), device="cuda", generator=gen) < 0.98
    g = torch.randn((N, H, W, 2), device="cuda", generator=gen) / (N * H * W)
    da, db = torch.empty_like(ab), torch.empty_like(bc)
    npix = N * H * W
    res = {"what": "compose_flows / compose_grad beside a torch grid_sample restatement (context only); medians",
           "command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:]),
           "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "shape": [N, H, W],
           "forward_bytes": 25 * npix, "forward_us_at_8TBps": 1e6 * 25 * npix / HBM_BYTES_PER_S}
    for key, kw in (("no_masks", {}), ("both_masks", dict(valid_ab=va, valid_bc=vb))):
        out, valid = P.compose_flows(ab, bc, **kw)
        res[f"valid_share_{key}"] = float(valid.float().mean())
        for name, fn in (("forward", lambda: P.compose_flows(ab, bc, **kw)),
                         ("grad", lambda: P.compose_grad(ab, bc, g, dflow_ab=da, dflow_bc=db, **kw))):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms, mm = events_ms(fn, args.iters, args.repeats)
            res[f"{name}_{key}"] = {"us": 1e3 * ms, "us_min_max": [1e3 * t for t in mm]}
    # the grid_sample route, forward and forward + backward into both flows
    out, ok = P.compose_flows(ab, bc)
    res["grid_sample_max_abs_difference_at_valid"] = float((grid_sample_compose(ab, bc) - out)[ok].abs().max())
    a, b = ab.clone().requires_grad_(True), bc.clone().requires_grad_(True)

    def torch_step():
        a.grad = b.grad = None
        grid_sample_compose(a, b).backward(g)

    for name, fn in (("forward", lambda: grid_sample_compose(ab, bc)), ("forward_backward", torch_step)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms, mm = events_ms(fn, args.iters, args.repeats)
        res[f"grid_sample_{name}"] = {"us": 1e3 * ms, "us_min_max": [1e3 * t for t in mm]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time filter_flow (pwcnet_amd/flow_filter.py) at 8 x 448 x 1024 with a uint8 guide for r = 1, 2, 3 and 7 (one pass) and for
three passes at r = 2, and fill_flow at r = 2 over a field with holes.  Device events around windows of calls through the Python
API (table upload and allocations included), warm-up first, the cases alternating, several repeats; medians.  Beside it a torch
restatement of one pass at r = 2 on the same GPU -- unfold, sort, gather, cumsum, first index whose doubled cumulative weight
reaches the total -- as the baseline a user could write today; it is context, nothing is asserted.  Also the LDS reads of the
selection per pixel, (rounds) x (2r+1)^2 x (dwords per candidate), the number DESIGN.md 23 reasons with.  Prints one JSON line (and
writes it to --out).

    python scripts/bench_flow_filter.py [--shape 8 448 1024] [--repeats 7] [--iters 5] [--out profiles/flow_filter_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_baseline(flows, guide, space, color, r):
    """One smoothing pass, every pixel known: the lower weighted median per component by sorting every window."""
    import torch.nn.functional as F
    N, H, W, _ = flows.shape
    D = 2 * r + 1
    inside = F.unfold(torch.ones((N, 1, H, W), device=flows.device), D, padding=r)                      # (N, D D, H W)
    g = guide.permute(0, 3, 1, 2).float()
    gw = F.unfold(g, D, padding=r).view(N, 3, D * D, H * W)
    d = (gw - g.reshape(N, 3, 1, H * W)).abs().sum(dim=1).long()                                        # (N, D D, H W)
    w = space.double().view(1, D * D, 1) * color.double()[d] * inside.double()
    total = w.sum(dim=1, keepdim=True)
    out = []
    for c in range(2):
        v = F.unfold(flows[..., c].unsqueeze(1), D, padding=r)
        vs, order = torch.sort(v, dim=1)
        cum = torch.cumsum(torch.gather(w, 1, order), dim=1)
        first = (2.0 * cum >= total).to(torch.uint8).argmax(dim=1, keepdim=True)
        out.append(torch.gather(vs, 1, first).view(N, H, W))
    return torch.stack(out, dim=3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_filter.py needs a GPU")
    import pwcnet_amd as P
    N, H, W = args.shape
    rs = np.random.RandomState(0)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flows = np.empty((N, H, W, 2))
    for n in range(N):                      # a camera motion, 0.3 px of noise, a rectangle moving on its own
        flows[n, ..., 0] = 2.0 + 0.01 * n * (x - W / 2) - 0.004 * (y - H / 2)
        flows[n, ..., 1] = -1.0 + 0.004 * (x - W / 2) + 0.01 * n * (y - H / 2)
    flows += rs.normal(0, 0.3, flows.shape)
    flows[:, H // 3:H // 3 + H // 5, W // 4:W // 4 + W // 5] += (8.0, -6.0)
    guide = np.clip(96 + 0.1 * x[None, ..., None] + rs.normal(0, 6, (N, H, W, 3)), 0, 255)
    guide[:, H // 3:H // 3 + H // 5, W // 4:W // 4 + W // 5] += 80
    flows = torch.from_numpy(flows.astype(np.float32)).cuda()
    guide = torch.from_numpy(np.clip(guide, 0, 255).astype(np.uint8)).cuda()
    holes = torch.from_numpy(rs.uniform(size=(N, H, W)) < 0.9).cuda()           # 10 % unknown, single pixels mostly
    sig = dict(sigma_space=2.0, sigma_color=10.0)

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    runs = {f"filter_r{r}": (lambda r=r: P.filter_flow(flows, guide=guide, radius=r, **sig)) for r in (1, 2, 3, 7)}
    runs["filter_r2_iters3"] = lambda: P.filter_flow(flows, guide=guide, radius=2, iters=3, **sig)
    runs["filter_r2_no_guide"] = lambda: P.filter_flow(flows, radius=2, sigma_space=2.0)
    runs["fill_r2_iters2"] = lambda: P.fill_flow(flows, valid=holes, guide=guide, radius=2, iters=2, **sig)
    space, color = (torch.from_numpy(t.astype(np.int64)).cuda() for t in P.filter_tables(2, 2.0, 10.0, 3))
    runs["torch_unfold_sort_r2"] = lambda: torch_baseline(flows, guide, space, color, 2)
    for fn in runs.values():                # warm-up
        fn()
    torch.cuda.synchronize()
    ours = P.filter_flow(flows, guide=guide, radius=2, **sig)[0]
    agree = float((ours == runs["torch_unfold_sort_r2"]()).float().mean())
    left = int((~runs["fill_r2_iters2"]()[1]).sum())
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, 1 if key.startswith("torch") else args.iters))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    # the selection's LDS reads per pixel: r = 1 reads its 9 cells once (3 dwords each, the rest is registers); r = 2, 3 read
    # the guide dword once per cell and two keys per cell and round; r >= 4 reads three dwords and a colour entry per cell and round
    lds = {1: 9 * 3, 2: 25 * (1 + 2 * 32), 3: 49 * (1 + 2 * 32), 7: 225 * 4 * 33}
    npix = N * H * W
    res = {"what": "filter_flow / fill_flow, ms per call (device events, medians of alternating windows of calls through the Python "
                   "API, table upload and allocations included), uint8 guide with three channels, sigma_space 2, sigma_color 10; "
                   "torch_unfold_sort_r2 = one pass at r = 2 restated with torch unfold + sort + cumsum on the same GPU (context; "
                   "baseline_agreement = the share of its values equal to filter_flow's); lds_dwords_per_pixel = the selection's LDS "
                   "reads; lds_dwords_per_ns = those over the measured time",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()}, "baseline_agreement": agree,
           "unknown_left_after_fill": left, "lds_dwords_per_pixel": lds,
           "lds_dwords_per_ns": {f"filter_r{r}": lds[r] * npix / (med[f"filter_r{r}"] * 1e6) for r in (1, 2, 3, 7)},
           "not_measured": "the launches alone (no profiler run), any other shape, any effect on flow error",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

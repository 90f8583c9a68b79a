#!/usr/bin/env python
"""Time label_regions (pwcnet_amd/regions.py) at 8 x 448 x 1024 for both connectivities, with and without flows, on two inputs:
the motion_residual inlier mask of a rectangle scene (inverted: one large region, the common case) and a Bernoulli p = 0.6 mask
(the ragged case: thousands of components, every seam busy).  Device events around windows of calls, warm-up first, the cases
alternating, several repeats; medians.  Beside it, where scipy is importable, scipy.ndimage.label on the host with the transfers a
user pays today (mask down, labels up), one image at a time: context, not a target.  Also the bytes each launch must move and what
fraction of 8 TB/s the whole call achieves against their sum.  Prints one JSON line (and writes it to --out).

    python scripts/bench_regions.py [--shape 8 448 1024] [--repeats 7] [--iters 5] [--out profiles/regions_bench.json]
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
PEAK = 8.0e12


def must_move(npix, fg, flows):
    """Bytes per launch that cannot be avoided with this launch plan (gathers counted once, the seam lanes and tables left out)."""
    b = {"tile": npix * (1 + 4 + 4) + (8 * fg if flows else 0),      # mask in, link and the zeroed areas out, the flow of masked-in pixels
         "flatten": npix * (4 + 4),                                   # link in, root out
         "area": npix * 4,                                            # root in
         "count": npix * 4, "number": npix * 4,                       # root in (areas only at the roots)
         "final": npix * (4 + 4) + fg * 4 + (8 * fg if flows else 0)}  # root in, labels out, the id gather, the flow of labelled pixels
    b["total"] = sum(b.values())
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_regions.py needs a GPU")
    import pwcnet_amd as P
    N, H, W = args.shape
    rs = np.random.RandomState(0)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    flows = np.empty((N, H, W, 2))
    for n in range(N):                      # a camera motion, 0.05 px of noise, a rectangle moving on its own
        flows[n, ..., 0] = 2.0 + 0.01 * n * (x - W / 2) - 0.004 * (y - H / 2)
        flows[n, ..., 1] = -1.0 + 0.004 * (x - W / 2) + 0.01 * n * (y - H / 2)
    flows += rs.normal(0, 0.05, flows.shape)
    flows[:, H // 3:H // 3 + H // 5, W // 4:W // 4 + W // 5] += (8.0, -6.0)
    flows = torch.from_numpy(flows.astype(np.float32)).cuda()
    matrices = P.fit_motion(flows, model="affine", iters=4)[0]
    residual, inlier = P.motion_residual(flows, matrices)
    moving = ~inlier                                                  # (so that both inputs run with invert=False)
    ragged = torch.from_numpy(rs.uniform(size=(N, H, W)) < 0.6).cuda()
    inputs = {"rectangle": moving, "bernoulli0.6": ragged}

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    runs, counts = {}, {}
    for name, mask in inputs.items():
        for c in (4, 8):
            for with_flows in (False, True):
                key = f"{name}_c{c}_{'flows' if with_flows else 'mask'}"
                runs[key] = lambda mask=mask, c=c, f=(residual if with_flows else None): P.label_regions(mask, connectivity=c, flows=f)
    for key, fn in runs.items():                # warm-up
        fn()
        counts[key] = fn()[1].cpu().numpy().tolist()
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, args.iters))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    npix = N * H * W
    moved, fraction = {}, {}
    for name, mask in inputs.items():
        fg = int(mask.sum())
        for with_flows in (False, True):
            tag = "flows" if with_flows else "mask"
            moved[f"{name}_{tag}"] = must_move(npix, fg, with_flows)
            for c in (4, 8):
                fraction[f"{name}_c{c}_{tag}"] = moved[f"{name}_{tag}"]["total"] / (med[f"{name}_c{c}_{tag}"] * 1e-3) / PEAK
    host = None
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    if ndimage is not None:                 # one pass is enough: it is three orders of magnitude away
        host = {}
        for name, mask in inputs.items():
            for c in (4, 8):
                structure = np.ones((3, 3), int) if c == 8 else None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = mask.cpu().numpy()
                out = np.stack([ndimage.label(m[n], structure=structure)[0] for n in range(N)])
                torch.from_numpy(out).cuda()
                torch.cuda.synchronize()
                host[f"{name}_c{c}"] = 1e3 * (time.perf_counter() - t0)
    res = {"what": "label_regions, ms per call (device events, medians of alternating windows of calls through the Python API, "
                   "allocations included): <input>_c<connectivity>_<mask alone | with flows>; must_move_bytes = what each launch "
                   "cannot avoid reading and writing; fraction_of_8TBps = their sum over the whole call's time; "
                   "scipy_host_ms = scipy.ndimage.label image by image with the mask copied down and the labels copied up, one "
                   "pass (context, labels only: no areas, boxes or means)",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()}, "regions_per_image": counts,
           "must_move_bytes": moved, "fraction_of_8TBps": fraction, "scipy_host_ms": host,
           "not_measured": "the launches one by one (no profiler run), the seam launch's atomics, any other shape",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

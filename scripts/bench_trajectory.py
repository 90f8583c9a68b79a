#!/usr/bin/env python
"""Time the scale chain at 8 x 448 x 1024: camera_trajectory and flow_trajectory beside a torch float64 route on the same GPU in the
same process (the triangulation again, a gather of the four corners, torch.kthvalue per seam, the running product on the host: the
route a user has without the ops -- context, not a target), and beside triangulate_depth and flow_depth alone.  The flows are the
sequence scene of tests/trajectory_ref.py at the bench's size, exact.  Device events around windows of calls, warm-up first, the
routes alternating, several repeats; medians.  Also the scale error against the scene's own and the largest difference between the
ops' and the torch route's ratios.  Prints one JSON line (and writes it to --out).

    python scripts/bench_trajectory.py [--shape 8 448 1024] [--repeats 5] [--iters 5] [--out profiles/trajectory_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_links(flows, R, t, K, depth, known):
    """The seams' ratios and sample counts with torch float64 ops: (ratio (T,) float32, samples (T,) long), index 0 empty."""
    from scripts.bench_pose import _rays, _triangulate
    T, H, W, _ = flows.shape
    xs, ys, qx, qy, d0, d1 = _rays(flows[:-1], K[:-1])
    _, den, _, z1 = _triangulate(R[:-1], t[:-1], d0, d1)
    inside = (qx >= 0) & (qx <= W - 1) & (qy >= 0) & (qy <= H - 1)
    fx0, fy0 = qx.clamp(0, W - 1).floor(), qy.clamp(0, H - 1).floor()
    x0, y0 = fx0.long(), fy0.long()
    x1, y1 = (x0 + 1).clamp(max=W - 1), (y0 + 1).clamp(max=H - 1)
    D, Kn = depth[1:].reshape(T - 1, H * W).double(), known[1:].reshape(T - 1, H * W)
    corner = [(y0 * W + x0), (y0 * W + x1), (y1 * W + x0), (y1 * W + x1)]
    c = [D.gather(1, o.reshape(T - 1, -1)).reshape(T - 1, H, W) for o in corner]
    k4 = torch.stack([Kn.gather(1, o.reshape(T - 1, -1)).reshape(T - 1, H, W) for o in corner]).all(0)
    wx1, wy1 = qx - fx0, qy - fy0
    d = (1 - wy1) * ((1 - wx1) * c[0] + wx1 * c[1]) + wy1 * ((1 - wx1) * c[2] + wx1 * c[3])
    r = (z1 / d).float()
    sample = known[:-1] & inside & k4 & (den > 0) & (z1 > 0) & (d > 0) & torch.isfinite(r) & (r > 0)
    ratio = torch.zeros(T, dtype=torch.float32, device=flows.device)
    samples = torch.zeros(T, dtype=torch.long, device=flows.device)
    for j in range(1, T):
        v = r[j - 1][sample[j - 1]]
        n = v.numel()
        samples[j] = n
        if n:
            ratio[j] = torch.kthvalue(v, (n - 1) // 2 + 1).values
    return ratio, samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("T", "H", "W"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window (the torch route: one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trajectory.py needs a GPU")
    import pwcnet_amd as P
    from tests import trajectory_ref as R
    T, H, W = args.shape
    scene = R.sequence(T, H, W)
    flows = torch.from_numpy(scene["flows"]).cuda()
    K = torch.from_numpy(np.tile(scene["K"], (T, 1))).cuda()

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    depth, known, rot, tra, ok, dinfo = P.flow_depth(flows, K)
    inl = dinfo["inlier"]
    traj, scales, segment, info, _ = P.camera_trajectory(flows, rot, tra, K, depth, known)
    runs = {
        "camera_trajectory": lambda: P.camera_trajectory(flows, rot, tra, K, depth, known),
        "camera_trajectory_two_pairs": lambda: P.camera_trajectory(flows[:2], rot[:2], tra[:2], K[:2], depth[:2], known[:2]),
        "flow_trajectory": lambda: P.flow_trajectory(flows, K),
        "flow_depth": lambda: P.flow_depth(flows, K),
        "triangulate_depth": lambda: P.triangulate_depth(flows, rot, tra, K, valid=inl),
        "torch_links": lambda: torch_links(flows, rot, tra, K, depth, known),
    }
    calls = {key: 1 if key.startswith("torch") else args.iters for key in runs}
    for fn in runs.values():                # warm-up
        fn()
        fn()
    tr, ts = torch_links(flows, rot, tra, K, depth, known)
    torch_scales = np.cumprod(np.concatenate([[1.0], tr[1:].double().cpu().numpy()]))          # the running product on the host
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, calls[key]))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    seams, npix = T - 1, float(H * W)
    res = {"what": "scale chain and camera trajectory, ms per call (device events, medians of alternating windows): camera_trajectory "
                   "(two memsets, keys, three selects, two histogram passes, the chain; and on two pairs of the batch), "
                   "flow_trajectory = flow_depth + camera_trajectory, flow_depth and triangulate_depth alone, torch_links = the "
                   "seams' medians with torch float64 ops (a gather per corner, kthvalue per seam, its count read on the host); "
                   "gbps = the bytes the launches of camera_trajectory must move (keys: 8 + 1 read, 4 corners x 5 read, 4 written; "
                   "two histogram passes: 4 read each; per seam pixel 41) over the call's time -- the launches were not separated",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "gbps": {"camera_trajectory": 41.0 * seams * npix / (med["camera_trajectory"] * 1e-3) / 1e9},
           "ok": [bool(v) for v in ok.cpu().numpy()], "ratio": info["ratio"].cpu().numpy().tolist(),
           "samples": info["samples"].cpu().numpy().tolist(), "linked": [bool(v) for v in info["linked"].cpu().numpy()],
           "scales": scales.cpu().numpy().tolist(), "segment": segment.cpu().numpy().tolist(),
           "scale_error": R.scale_error(scales.cpu().numpy(), T), "unit_scale_error": R.scale_error(np.ones(T), T),
           "last_centre_error": R.centre_error(traj[T].cpu().numpy(), T), "unit_last_centre_error": R.unit_centre_error(T),
           "largest_difference_op_vs_torch": {"ratio_relative": float(((info["ratio"] - tr).abs()[1:] / tr[1:]).max()),
                                              "samples_differ": int((info["samples"].long() != ts).sum()),
                                              "scales_relative": float(np.abs(scales.cpu().numpy() / torch_scales - 1.0).max())},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

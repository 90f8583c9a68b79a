#!/usr/bin/env python
"""Time the pose path at 8 x 448 x 1024: camera_pose, triangulate_depth and flow_depth beside a torch float64 restatement on the
same GPU in the same process (torch.linalg.svd of E, four batched triangulations, argmax: the route a user has without the ops --
context, not a target), and triangulate_depth beside epipolar_residual, which streams the same bytes.  The flows are the test
scene of tests/fundamental_ref.py at the bench's size with 0.05 px of noise.  Device events around windows of calls, warm-up
first, the routes alternating, several repeats; medians.  Also the pose error against the scene's own and the largest difference
between the ops' and the torch route's rotation, translation and depth.  Prints one JSON line (and writes it to --out).

    python scripts/bench_pose.py [--shape 8 448 1024] [--repeats 5] [--iters 5] [--out profiles/pose_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _rays(flows, K):
    N, H, W, _ = flows.shape
    dev = flows.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    fx, fy, cx, cy = (K[:, j].reshape(N, 1, 1) for j in range(4))
    xp, yp = xs + flows[..., 0].double(), ys + flows[..., 1].double()
    one = torch.ones_like(xp)
    d0 = torch.stack([((xs - cx) / fx).expand_as(xp), ((ys - cy) / fy).expand_as(xp), one], -1)
    d1 = torch.stack([(xp - cx) / fx, (yp - cy) / fy, one], -1)
    return xs, ys, xp, yp, d0, d1


def _triangulate(R, t, d0, d1):
    """(a, den, Z0, Z1) for R (N,3,3), t (N,3), rays (N,H,W,3)."""
    a = torch.einsum("nij,nhwj->nhwi", R, d0)
    c = torch.linalg.cross(d1, a)
    e = torch.linalg.cross(d1, t[:, None, None, :].expand_as(d1))
    den = (c * c).sum(-1)
    z0 = -(c * e).sum(-1) / den
    return a, den, z0, z0 * a[..., 2] + t[:, None, None, 2]


def torch_pose(flows, F, K, threshold):
    """camera_pose with torch float64 ops: svd, four batched triangulations, argmax.  (R, t)."""
    N = flows.shape[0]
    Km = torch.zeros((N, 3, 3), dtype=torch.float64, device=flows.device)
    Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2], Km[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1.0
    E = Km.transpose(1, 2) @ F @ Km
    U, _, Vt = torch.linalg.svd(E)
    U = U * torch.sign(torch.linalg.det(U)).reshape(N, 1, 1)
    Vt = Vt * torch.sign(torch.linalg.det(Vt)).reshape(N, 1, 1)
    Wm = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float64, device=flows.device)
    Ra, Rb, t = U @ Wm @ Vt, U @ Wm.T @ Vt, U[:, :, 2]
    xs, ys, xp, yp, d0, d1 = _rays(flows, K)
    p = torch.stack([xs.expand_as(xp), ys.expand_as(xp), torch.ones_like(xp)], -1)
    q = torch.stack([xp, yp, torch.ones_like(xp)], -1)
    l, lp = torch.einsum("nij,nhwj->nhwi", F, p), torch.einsum("nji,nhwj->nhwi", F, q)
    r = (q * l).sum(-1)
    g = l[..., 0] ** 2 + l[..., 1] ** 2 + lp[..., 0] ** 2 + lp[..., 1] ** 2
    voter = (g > 0) & (r.abs() / g.sqrt() <= threshold)
    votes = []
    for R, tt in ((Ra, t), (Ra, -t), (Rb, t), (Rb, -t)):
        _, den, z0, z1 = _triangulate(R, tt, d0, d1)
        votes.append((voter & (den > 0) & (z0 > 0) & (z1 > 0)).sum(dim=(1, 2)))
    win = torch.stack(votes, 1).argmax(1)
    R = torch.where((win < 2).reshape(N, 1, 1), Ra, Rb)
    return R, torch.where((win % 2 == 0).reshape(N, 1), t, -t)


def torch_depth(flows, R, t, K, valid, min_parallax):
    """triangulate_depth with torch float64 ops: (depth float32, known)."""
    xs, ys, xp, yp, d0, d1 = _rays(flows, K)
    a, den, z0, z1 = _triangulate(R, t, d0, d1)
    N = flows.shape[0]
    fx, fy, cx, cy = (K[:, j].reshape(N, 1, 1) for j in range(4))
    par = ((xp - (fx * a[..., 0] / a[..., 2] + cx)) ** 2 + (yp - (fy * a[..., 1] / a[..., 2] + cy)) ** 2).sqrt()
    known = valid & (a[..., 2] > 0) & (den > 0) & (z0 > 0) & (z1 > 0) & (par >= min_parallax)
    return torch.where(known, z0.float(), torch.full_like(z0, 1e10, dtype=torch.float32)), known


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window (the torch routes: one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose.py needs a GPU")
    import pwcnet_amd as P
    from tests import fundamental_ref as FR
    from tests import pose_ref as R
    N, H, W = args.shape
    flows = torch.from_numpy(np.stack([FR.scene(H, W, n, True, 0.05)[0] for n in range(N)])).cuda()
    K = torch.from_numpy(np.tile(R.scene_intrinsics(H, W), (N, 1))).cuda()

    def window(fn, iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters

    fund, fok, _ = P.fit_fundamental(flows, iters=4)
    dist, inl = P.epipolar_residual(flows, fund)
    rot, tra, ok, info = P.camera_pose(flows, fund, K)
    depth, known, par = P.triangulate_depth(flows, rot, tra, K, valid=inl, return_parallax=True)
    runs = {
        "camera_pose": lambda: P.camera_pose(flows, fund, K),
        "camera_pose_one_image": lambda: P.camera_pose(flows[:1], fund[:1], K[:1]),
        "triangulate_depth": lambda: P.triangulate_depth(flows, rot, tra, K, valid=inl),
        "triangulate_depth_with_parallax": lambda: P.triangulate_depth(flows, rot, tra, K, valid=inl, return_parallax=True),
        "epipolar_residual": lambda: P.epipolar_residual(flows, fund),
        "fit_fundamental": lambda: P.fit_fundamental(flows, iters=4),
        "flow_depth": lambda: P.flow_depth(flows, K),
        "torch_pose": lambda: torch_pose(flows, fund, K, 1.0),
        "torch_depth": lambda: torch_depth(flows, rot, tra, K, inl, 0.25),
    }
    calls = {key: 1 if key.startswith("torch") else args.iters for key in runs}
    for fn in runs.values():                # warm-up
        fn()
        fn()
    tr, tt = torch_pose(flows, fund, K, 1.0)
    td, tk = torch_depth(flows, rot, tra, K, inl, 0.25)
    both = known & tk
    differ = {"rotation": float((rot - tr).abs().max()), "translation": float((tra - tt).abs().max()),
              "depth_relative": float(((depth - td).abs() / td.abs())[both].max()), "known_differ": int((known != tk).sum())}
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, calls[key]))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    npix = float(N * H * W)
    rot_err = [R.rotation_error(r, R.scene_rotation()) for r in rot.cpu().numpy()]
    tra_err = [R.direction_error(t, R.scene_translation()) for t in tra.cpu().numpy()]
    static = torch.from_numpy(~FR.block_mask(H, W)).cuda()[None] & known
    rel = (depth.double() / torch.from_numpy(R.scene_depth(H, W)).cuda()[None] - 1.0).abs()[static]
    res = {"what": "relative pose and depth, ms per call (device events, medians of alternating windows): camera_pose (decompose, vote, "
                   "select; and on one image of the batch), triangulate_depth (with valid = inlier; and with the parallax output) "
                   "beside epipolar_residual, flow_depth = fit_fundamental + epipolar_residual + camera_pose + triangulate_depth, "
                   "torch_pose / torch_depth = the same with torch float64 ops (svd, four batched triangulations, argmax); "
                   "gbps = the bytes a launch must move (depth: 8 + 1 read, 5 written per pixel; vote: 8 read) over the call's time",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "gbps": {"triangulate_depth": 14.0 * npix / (med["triangulate_depth"] * 1e-3) / 1e9,
                    "epipolar_residual": 13.0 * npix / (med["epipolar_residual"] * 1e-3) / 1e9,
                    "camera_pose": 8.0 * npix / (med["camera_pose"] * 1e-3) / 1e9},
           "ok": [bool(v) for v in ok.cpu().numpy()], "votes": info["votes"].cpu().numpy().tolist(),
           "voters": info["voters"].cpu().numpy().tolist(), "singular": info["singular"].cpu().numpy().tolist(),
           "rotation_error_deg": rot_err, "translation_error_deg": tra_err,
           "known_share": float(known.float().mean()), "inlier_share": float(inl.float().mean()),
           "static_relative_depth_error_median_max": [float(rel.median()), float(rel.max())],
           "parallax_px_min_median": [float(par[known].min()), float(par[known].median())],
           "largest_difference_op_vs_torch": differ, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

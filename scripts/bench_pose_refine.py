#!/usr/bin/env python
"""Time the pose refinement at 8 x 448 x 1024: refine_pose at iters = 4 beside a torch float64 loop of the same Gauss-Newton on the
same GPU in the same process (batched tensor ops, torch.linalg.solve, the best pass kept with torch.where: the route a user has
without the op -- context, not a target), and flow_depth(refine=4) beside flow_depth().  The flows are the bench scene of
scripts/bench_pose.py: the test scene of tests/fundamental_ref.py at the bench's size with 0.05 px of noise.  Device events around
windows of calls, warm-up first, the routes alternating, several repeats; medians.  No time is set in advance.  The expectation to
confirm or refute: a pass costs about one cheirality-vote launch of camera_pose plus a one-lane solve, so flow_depth(refine=4)
stays within a few percent of flow_depth(), whose time is fit_fundamental's.  Also the pose error against the scene's own before
and after, and the largest difference between the op's and the torch loop's pose.  Prints one JSON line (and writes it to --out).

    python scripts/bench_pose_refine.py [--shape 8 448 1024] [--repeats 5] [--iters 5] [--out profiles/pose_refine_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _terms(flows, R, t, K):
    """(a, c, e, r, g) of every pixel under (R (N,3,3), t (N,3)): the epipolar residual on the rays and its gradient in pixels."""
    N, H, W, _ = flows.shape
    dev = flows.device
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64),
                            indexing="ij")
    fx, fy, cx, cy = (K[:, j].reshape(N, 1, 1) for j in range(4))
    xp, yp = xs + flows[..., 0].double(), ys + flows[..., 1].double()
    one = torch.ones_like(xp)
    d0 = torch.stack([((xs - cx) / fx).expand_as(xp), ((ys - cy) / fy).expand_as(xp), one], -1)
    d1 = torch.stack([(xp - cx) / fx, (yp - cy) / fy, one], -1)
    a = torch.einsum("nij,nhwj->nhwi", R, d0)
    tt = t[:, None, None, :].expand_as(d1)
    c, e = torch.linalg.cross(d1, a), torch.linalg.cross(d1, tt)
    r = (e * a).sum(-1)
    l = torch.linalg.cross(tt, a)
    m = torch.einsum("nji,nhwj->nhwi", R, e)
    g = (l[..., 0] / fx) ** 2 + (l[..., 1] / fy) ** 2 + (m[..., 0] / fx) ** 2 + (m[..., 1] / fy) ** 2
    return a, c, e, r, g


def _basis(t):
    axis = torch.nn.functional.one_hot(t.abs().argmin(dim=1), 3).to(t.dtype)
    b1 = torch.linalg.cross(axis, t)
    b1 = b1 / b1.norm(dim=1, keepdim=True)
    return b1, torch.linalg.cross(t, b1)


def torch_refine(flows, R0, t0, K, iters, scale, threshold):
    """refine_pose with torch float64 ops: the same pixel set, weights, fixed-g Jacobian, Cayley and tangent updates, best pass."""
    N = flows.shape[0]
    _, _, _, r, g = _terms(flows, R0, t0, K)
    inset = (g > 0) & (r.abs() / g.sqrt() <= threshold)
    R, t = R0, t0
    best_R, best_t, best_cost = R0, t0, None
    eye = torch.eye(3, dtype=torch.float64, device=flows.device)
    for it in range(iters + 1):
        a, c, e, r, g = _terms(flows, R, t, K)
        sg = g.sqrt()
        d2 = r * r / g
        w = torch.where(inset, 1.0 / (1.0 + d2 / (scale * scale)), torch.zeros_like(d2))
        cost = (w * d2).sum(dim=(1, 2))
        if best_cost is None:
            best_cost = cost
        else:
            better = cost < best_cost
            best_R, best_t = torch.where(better[:, None, None], R, best_R), torch.where(better[:, None], t, best_t)
            best_cost = torch.where(better, cost, best_cost)
        if it == iters:
            break
        b1, b2 = _basis(t)
        J = torch.cat([torch.linalg.cross(a, e), -(c * b1[:, None, None, :]).sum(-1, keepdim=True),
                       -(c * b2[:, None, None, :]).sum(-1, keepdim=True)], -1) / sg[..., None]
        wJ = w[..., None] * J
        A = torch.einsum("nhwi,nhwj->nij", wJ, J)
        b = torch.einsum("nhwi,nhw->ni", wJ, r / sg)
        x = torch.linalg.solve(A, -b)
        h = x[:, :3] / 2.0
        q = (h * h).sum(1).reshape(N, 1, 1)
        zero = torch.zeros_like(h[:, 0])
        skew = torch.stack([zero, -h[:, 2], h[:, 1], h[:, 2], zero, -h[:, 0], -h[:, 1], h[:, 0], zero], 1).reshape(N, 3, 3)
        C = ((1.0 - q) * eye + 2.0 * h[:, :, None] * h[:, None, :] + 2.0 * skew) / (1.0 + q)
        R = C @ R
        u = t + x[:, 3:4] * b1 + x[:, 4:5] * b2
        t = u / u.norm(dim=1, keepdim=True)
    return best_R, best_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5, help="calls per timed window (the torch route: one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_refine.py needs a GPU")
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
    rot, tra, ok, _ = P.camera_pose(flows, fund, K)
    rot2, tra2, rok, info = P.refine_pose(flows, rot, tra, K, iters=4)
    runs = {
        "refine_pose": lambda: P.refine_pose(flows, rot, tra, K, iters=4),
        "refine_pose_iters_0": lambda: P.refine_pose(flows, rot, tra, K, iters=0),
        "refine_pose_one_image": lambda: P.refine_pose(flows[:1], rot[:1], tra[:1], K[:1], iters=4),
        "camera_pose": lambda: P.camera_pose(flows, fund, K),
        "fit_fundamental": lambda: P.fit_fundamental(flows, iters=4),
        "flow_depth": lambda: P.flow_depth(flows, K),
        "flow_depth_refine_4": lambda: P.flow_depth(flows, K, refine=4),
        "torch_refine": lambda: torch_refine(flows, rot, tra, K, 4, 1.0, 1.0),
    }
    calls = {key: 1 if key.startswith("torch") else args.iters for key in runs}
    for fn in runs.values():                # warm-up
        fn()
        fn()
    tr, tt = torch_refine(flows, rot, tra, K, 4, 1.0, 1.0)
    differ = {"rotation": float((rot2 - tr).abs().max()), "translation": float((tra2 - tt).abs().max())}
    torch.cuda.synchronize()
    ms = {key: [] for key in runs}
    for _ in range(args.repeats):
        for key, fn in runs.items():
            ms[key].append(window(fn, calls[key]))
    med = {key: float(np.median(t)) for key, t in ms.items()}
    npix = float(N * H * W)

    def errors(r, t):
        return ([R.rotation_error(q, R.scene_rotation()) for q in r.cpu().numpy()],
                [R.direction_error(q, R.scene_translation()) for q in t.cpu().numpy()])

    closed, refined = errors(rot, tra), errors(rot2, tra2)
    cost, best = info["cost"].cpu().numpy(), info["best_pass"].cpu().numpy()
    res = {"what": "pose refinement, ms per call (device events, medians of alternating windows): refine_pose at iters = 4 (5 sums and 5 "
                   "solve launches; at iters = 0: one of each; and on one image of the batch) beside camera_pose (whose vote launch "
                   "streams the same bytes), fit_fundamental and flow_depth with and without refine = 4; torch_refine = the same "
                   "Gauss-Newton with torch float64 ops; per_pass_ms = (refine_pose - refine_pose_iters_0) / 4; gbps = 8 bytes per "
                   "pixel and pass over the call's time",
           "shape": args.shape, "repeats": args.repeats, "iters": args.iters, "ms": med,
           "ms_min_max": {key: [min(t), max(t)] for key, t in ms.items()},
           "per_pass_ms": (med["refine_pose"] - med["refine_pose_iters_0"]) / 4.0,
           "flow_depth_refine_over_plain": med["flow_depth_refine_4"] / med["flow_depth"],
           "torch_over_op": med["torch_refine"] / med["refine_pose"],
           "gbps": {"refine_pose": 5.0 * 8.0 * npix / (med["refine_pose"] * 1e-3) / 1e9},
           "ok": [bool(v) for v in rok.cpu().numpy()], "samples": info["samples"].cpu().numpy().tolist(),
           "best_pass": best.tolist(), "cost_first": cost[:, 0].tolist(), "cost_best": cost[np.arange(N), best].tolist(),
           "rotation_error_deg": {"closed": closed[0], "refined": refined[0]},
           "translation_error_deg": {"closed": closed[1], "refined": refined[1]},
           "largest_difference_op_vs_torch": differ, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

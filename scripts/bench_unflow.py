#!/usr/bin/env python
"""Time the two last terms of UnFlow's loss, forward + backward, on the HIP path against the float32 torch-op restatements
(tests/unflow_ref.py) of the same terms on the same GPU, at the training frame size: device events around whole forward + backward
passes, warm-up first, the two versions alternating, several repeats; medians.  The gradients of both are compared with the
float64 restatement's at the timed size (max-abs error over the largest element).  Also timed, HIP only: the consistency term
when EVERY forward pixel of an image points into one cell (all of them add into the same 8 accumulators), at the GPU test's size
and at the timed size -- the fixed-point scatter's worst case.  Prints one JSON line (and writes it to --out).

    python scripts/bench_unflow.py [--shape 8 448 1024] [--repeats 7] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def compare(hip, ref, ref64, repeats, iters, ref_iters):
    """Timings of hip against ref (alternating windows) and both gradients' errors against ref64's."""
    (lh, gh), (lr, gr) = hip(), ref()              # warm-up, and the two versions against each other
    hip(), ref()
    torch.cuda.synchronize()
    l64, g64 = ref64()
    errs = []
    for got in (gh, gr):
        errs.append(max(float((a.double() - b).abs().max()) / float(b.abs().max()) for a, b in zip(got, g64)))
    del g64
    torch.cuda.empty_cache()
    t_hip, t_ref = [], []
    for _ in range(repeats):
        t_hip.append(window(hip, iters))
        t_ref.append(window(ref, ref_iters))
    return {"hip_ms": float(np.median(t_hip)), "hip_ms_min_max": [min(t_hip), max(t_hip)],
            "torch_fp32_ms": float(np.median(t_ref)), "torch_fp32_ms_min_max": [min(t_ref), max(t_ref)],
            "speedup": float(np.median(t_ref) / np.median(t_hip)), "loss_hip": float(lh), "loss_torch_fp32": float(lr),
            "loss_float64": float(l64), "grad_err_hip_vs_float64": errs[0], "grad_err_torch_fp32_vs_float64": errs[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs=3, type=int, default=[8, 448, 1024], metavar=("N", "H", "W"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="forward + backward passes per timed window of the HIP path")
    ap.add_argument("--ref-iters", type=int, default=2, help="... of the torch restatement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_unflow.py needs a GPU")
    from pwcnet_amd import unsup
    from tests import unflow_ref as uf
    N, H, W = args.shape
    case = uf.build_case(N, H, W, flow_scale=1.0, seed=0, masked=True, noise=0.5)
    fw, bw = torch.from_numpy(case["fw"]).cuda(), torch.from_numpy(case["bw"]).cuda()
    vf, vb = torch.from_numpy(case["valid_fw"]).cuda(), torch.from_numpy(case["valid_bw"]).cuda()
    image = torch.from_numpy(np.random.RandomState(1).uniform(0, 1, (N, H, W, 3)).astype(np.float32)).cuda()

    def leaves(dt=torch.float32):
        return fw.detach().to(dt).requires_grad_(True), bw.detach().to(dt).requires_grad_(True)

    def cons_hip():
        a, b = leaves()
        loss = unsup.fb_consistency_loss(a, b, 1.0, vf, vb)
        loss.backward()
        return loss.detach(), (a.grad, b.grad)

    def cons_ref(dt=torch.float32):
        a, b = leaves(dt)
        s_a, c_a, _, s_b, c_b, _ = uf.fb_consistency_ref(a, b, 1.0, vf, vb)
        loss = (s_a.sum() + s_b.sum()) / (2 * (c_a.sum() + c_b.sum()).clamp(min=1)).to(dt)
        loss.backward()
        return loss.detach(), (a.grad, b.grad)

    def smooth_hip():
        a, _ = leaves()
        loss = unsup.smoothness_loss(a, image, order=2)
        loss.backward()
        return loss.detach(), (a.grad,)

    def smooth_ref(dt=torch.float32):
        a, _ = leaves(dt)
        loss = uf.smoothness2_ref(a, image.to(dt)).sum() / float(N * H * W)
        loss.backward()
        return loss.detach(), (a.grad,)

    res = {"what": "UnFlow's last two terms, forward + backward, ms per pass (device events, medians of alternating windows)",
           "shape": args.shape, "repeats": args.repeats, "iters": [args.iters, args.ref_iters],
           "fb_consistency_loss": compare(cons_hip, cons_ref, lambda: cons_ref(torch.float64), args.repeats, args.iters,
                                          args.ref_iters),
           "smoothness_loss_order2": compare(smooth_hip, smooth_ref, lambda: smooth_ref(torch.float64), args.repeats, args.iters,
                                             args.ref_iters)}

    # contention: every forward pixel of an image into one cell
    def contention(n, h, w, cell, iters):
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        one = np.zeros((n, h, w, 2))
        one[..., 0], one[..., 1] = cell[0] - xs, cell[1] - ys
        a0 = torch.from_numpy(one.astype(np.float32)).cuda()
        b0 = torch.from_numpy(np.random.RandomState(2).uniform(-1, 1, (n, h, w, 2)).astype(np.float32)).cuda()

        def run():
            a, b = a0.detach().requires_grad_(True), b0.detach().requires_grad_(True)
            unsup.fb_consistency_loss(a, b).backward()
            return b.grad

        first = run()
        run()
        torch.cuda.synchronize()
        times = [window(run, iters) for _ in range(args.repeats)]
        return {"shape": [n, h, w], "cell": list(cell), "hip_ms": float(np.median(times)), "hip_ms_min_max": [min(times), max(times)],
                "finite": bool(torch.isfinite(first).all()), "same_bits_again": bool(torch.equal(first, run()))}

    res["contention_test_case"] = contention(2, 23, 37, uf.CELL, args.iters)
    res["contention_timed_size"] = contention(N, H, W, (W / 2 + 0.3, H / 2 + 0.6), 2)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Time the two launches of pwcnet_amd.fit at the evaluation size: the fit of both frames of a batch (N x 436 x 1024 uint8 ->
448 x 1024 float32, 2 N frames in one launch) and the refit of its flow (448 x 1024 -> 436 x 1024), modes resize and pad.
Captured chains of launches replayed between device events, median of the repeats, as scripts/exp_resize_ab.py does.  Each
launch is set against (a) a torch.nn.functional.interpolate(..., align_corners=False) restatement of the same step on the
same GPU (uint8 -> float -> / 255 -> interpolate; interpolate -> * scale), timed the same way, and (b) its own bytes moved at
8 TB/s.  Then the headline `python bench.py` once: the default path does not go through the fit.  No time is a pass / fail
condition.  Prints one JSON line and writes it to --out.

    python scripts/bench_fit.py [--batch 8] [--size 436 1024] [--chain 12] [--repeats 7] [--no-headline] [--out profiles/fit_bench.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def chain(fn, n, reps):
    """us per call of fn: n calls captured into one graph, the graph replayed between device events, median of reps."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", nargs=2, type=int, default=[436, 1024], metavar=("H", "W"))
    ap.add_argument("--chain", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-headline", action="store_true", help="skip the run of bench.py")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fit.py needs a GPU")
    import torch.nn.functional as F
    from pwcnet_amd import _lib, fit
    L = _lib.lib()
    B, (H, W) = args.batch, args.size
    FH, FW = fit.ceil_to(H), fit.ceil_to(W)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rs = np.random.RandomState(0)
    frames = torch.from_numpy(rs.randint(0, 256, size=(2 * B, H, W, 3)).astype(np.uint8)).cuda()       # both frames of B pairs
    fitted = torch.empty((2 * B, FH, FW, 3), device="cuda")
    flow = torch.from_numpy(rs.normal(0, 3, size=(B, FH, FW, 2)).astype(np.float32)).cuda()
    refit = torch.empty((B, H, W, 2), device="cuda")
    scale = torch.tensor([W / FW, H / FH], device="cuda")
    fit_bytes = frames.numel() + 4 * fitted.numel()
    refit_bytes = 4 * flow.numel() + 4 * refit.numel()        # RESIZE reads every source cell; PAD reads H x W of them

    def torch_fit():
        x = frames.permute(0, 3, 1, 2).float() / 255.0
        return F.interpolate(x, size=(FH, FW), mode="bilinear", align_corners=False).permute(0, 2, 3, 1).contiguous()

    def torch_refit():
        y = F.interpolate(flow.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
        return (y.permute(0, 2, 3, 1) * scale).contiguous()

    res = {"what": "pwc_fit_frames_f32 (both frames of the batch, uint8 in) and pwc_refit_flow_f32, us per launch (captured chains, "
                   "device events, medians)", "batch": B, "frame": [H, W], "network": [FH, FW], "chain": args.chain,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "fit_bytes": fit_bytes, "fit_us_at_8TBps": 1e6 * fit_bytes / HBM_BYTES_PER_S,
           "refit_bytes": refit_bytes, "refit_us_at_8TBps": 1e6 * refit_bytes / HBM_BYTES_PER_S}
    for mode, code in (("resize", _lib.FIT_RESIZE), ("pad", _lib.FIT_PAD)):
        hip_fit = lambda: _lib.check(L.pwc_fit_frames_f32(p(frames), 1, p(fitted), 2 * B, H, W, FH, FW, code, _lib.current_stream()))
        hip_refit = lambda: _lib.check(L.pwc_refit_flow_f32(p(flow), p(refit), B, FH, FW, H, W, code, _lib.current_stream()))
        res[f"fit_{mode}_us"], res[f"fit_{mode}_us_min_max"] = chain(hip_fit, args.chain, args.repeats)
        res[f"refit_{mode}_us"], res[f"refit_{mode}_us_min_max"] = chain(hip_refit, args.chain, args.repeats)
        res[f"fit_{mode}_fraction_of_8TBps"] = res["fit_us_at_8TBps"] / res[f"fit_{mode}_us"]
        res[f"refit_{mode}_fraction_of_8TBps"] = res["refit_us_at_8TBps"] / res[f"refit_{mode}_us"]
        if mode == "resize":                                   # what the float32 torch restatement is off by, on the same data
            hip_fit(), hip_refit()
            res["fit_resize_max_abs_diff_vs_torch"] = float((fitted - torch_fit()).abs().max())
            res["refit_resize_max_abs_diff_vs_torch"] = float((refit - torch_refit()).abs().max())
    res["fit_torch_interpolate_us"], res["fit_torch_interpolate_us_min_max"] = chain(torch_fit, args.chain, args.repeats)
    res["refit_torch_interpolate_us"], res["refit_torch_interpolate_us_min_max"] = chain(torch_refit, args.chain, args.repeats)
    del frames, fitted, flow, refit
    torch.cuda.empty_cache()
    if not args.no_headline:
        # a fresh process (this one holds the GPU open; bench.py builds its own model): the default path, which has no fit in it
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, cwd=ROOT)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        if out.returncode != 0 or not lines:
            raise SystemExit(f"bench.py failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
        head = json.loads(lines[-1])
        res["headline_bench"] = {k: head[k] for k in ("metric", "value", "unit", "ms_per_step") if k in head}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

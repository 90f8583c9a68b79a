#!/usr/bin/env python
"""Time the self-supervision term (train.py --selfsup_weight, DESIGN.md "Self-supervision") against the flag off, which is the step
the parent commit runs:

  op     flow_distill_sums and flow_distill_grad alone at 16 x 256 x 320 inside 384 x 448 at offset (64, 64) (the 2N-stacked
         student of the step below), with UFlow's two masks, device events around chains of calls, median of the repeats;
  step   train.py's unsup_step + Adam at 4 x 384 x 448 with --photo census --occlusion fb, --selfsup_weight 0.3 --selfsup_crop 64
         against 0, host clock around synchronised groups of steps, median of the repeats; the flag-off step is timed twice, around
         the other, so that the spread of one configuration is on record next to the difference.

Expectation: the op reads 16 x 256 x 320 x (8 + 8 + 2) bytes = 24 MB (sums) and writes 10 MB more (gradient): a few us each at HBM
speed, so launch latency is what it costs.  The step adds one forward and backward at 256 x 320 / (384 x 448) = 0.48 of the
pixels, a crop launch, a second fb_valid and the op: roughly 1.5 x the flag-off step.  Nothing is asserted.  Prints one JSON line
and writes it to --out.

    python scripts/bench_selfsup.py [--iters 30] [--repeats 9] [--steps 5] [--no-step] [--out profiles/selfsup_bench.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

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


def op_times(iters, repeats):
    import pwcnet_amd as P
    N, h, w, H, W, offset = 16, 256, 320, 384, 448, (64, 64)
    g = torch.Generator(device="cuda").manual_seed(0)
    student = torch.randn((N, h, w, 2), device="cuda", generator=g)
    teacher = torch.randn((N, H, W, 2), device="cuda", generator=g)
    tv = torch.rand((N, H, W), device="cuda", generator=g) < 0.8
    ex = torch.rand((N, h, w), device="cuda", generator=g) < 0.8
    dsums = torch.ones((N,), device="cuda")
    dst = torch.empty_like(student)
    res = {"student": [N, h, w], "teacher": [N, H, W], "offset": list(offset)}
    for key, kw in (("no_masks", {}), ("both_masks", dict(teacher_valid=tv, exclude=ex))):
        for _ in range(3):
            P.flow_distill_sums(student, teacher, offset, **kw)
            P.flow_distill_grad(student, teacher, dsums, dst, offset, **kw)
        torch.cuda.synchronize()
        masks = (N * H * W + N * h * w) if kw else 0                   # an upper bound: the teacher's mask is read in the window only
        for name, fn, nbytes in (("sums", lambda: P.flow_distill_sums(student, teacher, offset, **kw), 16 * N * h * w + masks),
                                 ("grad", lambda: P.flow_distill_grad(student, teacher, dsums, dst, offset, **kw),
                                  24 * N * h * w + masks)):
            ms, mm = events_ms(fn, iters, repeats)
            res[f"{name}_{key}"] = {"us": 1e3 * ms, "us_min_max": [1e3 * t for t in mm], "bytes": nbytes,
                                    "us_at_8TBps": 1e6 * nbytes / HBM_BYTES_PER_S}
    return res


def step_times(steps, repeats):
    import pwcnet_amd as P
    from tests import util
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "train.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    N, H, W, C, weight = 4, 384, 448, 64, 0.3
    im0, im1 = (torch.from_numpy(a).cuda() for a in util.smooth_images(N, H, W))
    objective = P.UnsupObjective(photo="census", occlusion="fb")
    model = P.PWCDCNetModule()
    opt = torch.optim.Adam(model.parameters(), lr=1e-6)
    res = {"shape": [N, H, W], "student": [N, H - 2 * C, W - 2 * C], "selfsup_weight": weight, "photo": "census", "occlusion": "fb",
           "pixels_ratio": (H - 2 * C) * (W - 2 * C) / (H * W)}

    def step(w):
        opt.zero_grad(set_to_none=True)
        _, terms = train.unsup_step(model, objective, im0, im1, w, C)
        opt.step()
        return terms

    for w in (0.0, weight):
        for _ in range(3):
            terms = step(w)
    res["selfsup_share"] = terms["selfsup_share"]
    for key, w in (("off", 0.0), ("on", weight), ("off_again", 0.0)):
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(w)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0) / steps)
        res[f"step_ms_{key}"], res[f"step_ms_{key}_min_max"] = float(np.median(ts)), [float(min(ts)), float(max(ts))]
    off = 0.5 * (res["step_ms_off"] + res["step_ms_off_again"])
    res["step_ms_on_minus_off"] = res["step_ms_on"] - off
    res["step_on_over_off"] = res["step_ms_on"] / off
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the training step timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_selfsup.py needs a GPU")
    res = {"what": "flow distillation op alone, and the label-free step with --selfsup_weight on against off (the parent's step); medians",
           "command": "python " + " ".join([os.path.relpath(os.path.abspath(sys.argv[0]), ROOT)] + sys.argv[1:]),
           "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "op": op_times(args.iters, args.repeats)}
    if not args.no_step:
        res["step"] = step_times(args.steps, args.repeats)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

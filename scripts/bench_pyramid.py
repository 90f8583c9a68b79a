#!/usr/bin/env python
"""Time frame_pyramid (pwcnet_amd/pyramid.py, one launch for the five levels 1/4 .. 1/64) on uint8 and float32 frames at the
training batch 8 x 384 x 448 x 3 and at 16 x 448 x 1024 x 3, against a torch restatement in the same process: avg_pool2d(4)
followed by four avg_pool2d(2) on the float32 frames (five launches, float32 accumulation), plus the / 255 conversion for bytes.
Captured chains of launches replayed between device events, median of the repeats, as scripts/bench_fit.py does; the frames of
the larger size do not fit the caches between two launches of a chain.  Each time is set against the algorithmic bytes (the input
once, the five outputs once) at 8 TB/s.  The byte results are checked bit for bit against float64 block sums on the GPU at both
sizes (the sizes at which a workgroup's tile is more than one block wide).  Then the label-free step (PWCDCNetModule forward,
Charbonnier + 0.1 smoothness on flows_final, backward) at 4 x 384 x 448 with and without the five level terms, the run without
them timed twice, around the other, so that the spread of one configuration is on record next to the difference.  No time is a
pass / fail condition.  Prints one JSON line and writes it to --out.

    python scripts/bench_pyramid.py [--chain 20] [--repeats 9] [--steps 12] [--no-step] [--out profiles/pyramid_bench.json]
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
from scripts.bench_fit import HBM_BYTES_PER_S, chain  # noqa: E402

FACTORS = (64, 32, 16, 8, 4)
SIZES = ((8, 384, 448, 3), (16, 448, 1024, 3))


def torch_chain(x32):
    """The five-launch restatement on NHWC float32 frames (channels_last views: no copy)."""
    import torch.nn.functional as F
    x = F.avg_pool2d(x32.permute(0, 3, 1, 2), 4)
    outs = [x]
    for _ in range(4):
        x = F.avg_pool2d(x, 2)
        outs.append(x)
    return outs[::-1]


def block_means_f64(x32, f):
    N, H, W, C = x32.shape
    return (x32.double().reshape(N, H // f, f, W // f, f, C).sum(dim=(2, 4)) / float(f * f)).float()


def step_times(steps, repeats):
    """ms per label-free step at 4 x 384 x 448: without the level terms, with them, without them again."""
    from pwcnet_amd import PWCDCNetModule, frame_pyramid, level_flow_scale, photometric_loss, smoothness_loss
    from tests import util
    im0, im1 = (torch.from_numpy(a).cuda() for a in util.smooth_images(4, 384, 448))
    weights = (0.32, 0.08, 0.02, 0.01, 0.005)
    model = PWCDCNetModule(seed=3)
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)

    def step(levels):
        opt.zero_grad(set_to_none=True)
        final, pyr = model(im0, im1)
        loss = photometric_loss(im0, im1, final) + 0.1 * smoothness_loss(final, im0)
        if levels:
            p0, p1 = frame_pyramid(im0, FACTORS), frame_pyramid(im1, FACTORS)
            for l, fl in enumerate(pyr):
                s = level_flow_scale(fl, (384, 448))
                loss = loss + weights[l] * (photometric_loss(p0[l], p1[l], fl, flow_scale=s) + 0.1 * smoothness_loss(s * fl, p0[l]))
        loss.backward()
        opt.step()
        return loss

    def run(levels):
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(levels)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0) / steps)
        return float(np.median(ts)), [float(min(ts)), float(max(ts))]

    for levels in (False, True):                                  # warm up both shapes of the step
        for _ in range(3):
            step(levels)
    res = {}
    for key, levels in (("final_only", False), ("level_weights", True), ("final_only_again", False)):
        res[f"step_ms_{key}"], res[f"step_ms_{key}_min_max"] = run(levels)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chain", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--no-step", action="store_true", help="skip the label-free step timing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pyramid.py needs a GPU")
    from pwcnet_amd import frame_pyramid
    res = {"what": "frame_pyramid, five levels 1/4 .. 1/64 from one launch, against avg_pool2d(4) + 4 x avg_pool2d(2) (float32, plus "
                   "/ 255 for bytes): us per call (captured chains, device events, medians)", "chain": args.chain,
           "repeats": args.repeats, "device": torch.cuda.get_device_name(0), "sizes": {}}
    rs = np.random.RandomState(0)
    for N, H, W, C in SIZES:
        host = torch.from_numpy(rs.randint(0, 256, size=(N, H, W, C)).astype(np.uint8))
        u8, f32 = host.cuda(), (host.float() / 255).cuda()        # (the host's division: the float32 nearest v / 255)
        out_bytes = sum(4 * N * (H // f) * (W // f) * C for f in FACTORS)
        r = {}
        for kind, x, torch_fn in (("uint8", u8, lambda: torch_chain(u8.float() / 255)), ("float32", f32, lambda: torch_chain(f32))):
            nbytes = x.numel() * x.element_size() + out_bytes
            us, mm = chain(lambda: frame_pyramid(x, FACTORS), args.chain, args.repeats)
            tus, tmm = chain(torch_fn, args.chain, args.repeats)
            r[kind] = {"bytes": nbytes, "us_at_8TBps": 1e6 * nbytes / HBM_BYTES_PER_S, "hip_us": us, "hip_us_min_max": mm,
                       "hip_fraction_of_8TBps": 1e6 * nbytes / HBM_BYTES_PER_S / us, "torch_chain_us": tus,
                       "torch_chain_us_min_max": tmm, "torch_over_hip": tus / us}
        got = frame_pyramid(u8, FACTORS)
        r["uint8_bit_equal_to_float64_block_means"] = all(
            torch.equal(g.view(torch.int32), block_means_f64(f32, f).view(torch.int32)) for f, g in zip(FACTORS, got))
        r["torch_chain_max_abs_diff"] = max(float((g - t.permute(0, 2, 3, 1)).abs().max()) for g, t in zip(got, torch_chain(f32)))
        res["sizes"][f"{N}x{H}x{W}x{C}"] = r
        del u8, f32, got
        torch.cuda.empty_cache()
    if not args.no_step:
        res.update(step_times(args.steps, args.repeats))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

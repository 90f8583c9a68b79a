#!/usr/bin/env python
"""Sharded EPE evaluation on the HIP path (the validation step of reference
train.py:124-131 as a stand-alone tool).

    python evaluate.py --list pairs.txt [--resume model_600.ckpt] [--batch 8] [--save_dir out]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 evaluate.py --list ...

pairs.txt: one pair per line, `image_0 image_1 flow_gt.flo [mask.png]`.  Images are cropped to multiples
of 64 (reference test.py:13-17), scaled to [0,1]; the ground truth and the mask are cropped the same way.  --fit resize / pad
evaluate the WHOLE frame instead: the frames are uploaded as uint8, resized or padded to the next multiples of 64 on the GPU, the
flow is brought back to the frame's own grid and compared with the uncropped ground truth and mask.
Sparse ground truth: pixels whose .flo value is the "unknown" sentinel (|u| or |v| above 1e9, or not finite) are
left out of every number; the optional fourth column names an 8-bit mask image, non-zero = valid
(`--mask_is_invalid`: non-zero = INVALID, Sintel's invalid/ images).  The JSON line carries the masked EPE, KITTI's
Fl-all, the 1/3/5-px error rates and the EPE by motion magnitude (pwcnet_amd.losses.summarize_metrics).  KITTI's
16-bit flow PNGs are not read here: convert them to .flo plus a mask image first.
Pairs are sharded contiguously over the ranks (one process per GPU, RCCL only for the final
all-gather of the statistics / flows); rank 0 prints one JSON line.
--save_dir D --save_vis also writes, per index, D/<index>.png and D/<index>_gt.png -- prediction and ground truth colour-coded
with ONE radius, the ground truth's largest magnitude over its valid pixels, so the two compare side by side -- and
D/<index>_err.png, the error on the log colour scale of KITTI's development kit (blue: below the Fl-all threshold, red: an
outlier, black: no ground truth), all made on the GPU (pwcnet_amd.vis).
--flow_filter R filters every predicted flow before it is scored and saved: the weighted median over a (2 R + 1)^2 window,
R = 1 .. 7, guided by the first frame on the flow's grid (pwcnet_amd.filter_flow; after the refit where --fit is not crop), with
--flow_filter_sigma_space (pixels), --flow_filter_sigma_color (grey levels per channel) [a box, no colour term] and
--flow_filter_iters [1].  Running with and without it is how its effect on EPE and Fl-all is measured; nobody has yet.
"""
import argparse
import json
import os
import time

import numpy as np
import torch


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--list", required=True)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--save_dir", default=None, help="write every predicted flow as <index>.flo (rank 0, after the gather)")
    ap.add_argument("--save_vis", action="store_true",
                    help="with --save_dir: also write <index>.png and <index>_gt.png (the flows colour-coded with the ground truth's "
                         "largest valid magnitude) and <index>_err.png (KITTI's log-scale error map), made on the GPU")
    ap.add_argument("--mask_is_invalid", action="store_true",
                    help="the mask column's images mark INVALID pixels with non-zero values (Sintel's invalid/)")
    ap.add_argument("--fit", choices=("crop", "resize", "pad"), default="crop",
                    help="frames whose size is no multiple of 64: crop them, ground truth and mask too (reference), or resize / "
                         "pad them on the GPU and compare the flow on the frame's own grid [crop]")
    ap.add_argument("--normalize_features", action="store_true",
                    help="correlate layer-normalised feature maps (PWCDCNet(normalize_features=True)).  A checkpoint carries no marker for this: pass it exactly when the weights were trained with it")
    ap.add_argument("--norm_eps", type=float, default=1e-16, help="--normalize_features: epsilon under the square root [1e-16]")
    from pwcnet_amd.flow_filter import add_cli_arguments
    add_cli_arguments(ap)
    return ap


def main():
    ap = build_parser()
    args = ap.parse_args()
    if args.save_vis and not args.save_dir:
        ap.error("--save_vis requires --save_dir")
    from pwcnet_amd.flow_filter import check_cli_arguments
    filt = check_cli_arguments(ap, args)                          # filter_flow's keyword arguments, None without the flag

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cuda", local_rank)

    from PIL import Image
    import pwcnet_amd
    from pwcnet_amd import ckpt, flow_io, sharding

    pairs = [ln.split() for ln in open(args.list) if ln.strip() and not ln.startswith("#")]
    model = pwcnet_amd.PWCDCNet(range_check="sync", normalize_features=args.normalize_features, norm_eps=args.norm_eps)      # results are final when a call returns (fp16-range check + fp32 repeat)
    if args.resume:
        model.load_weights(ckpt.load_weights(args.resume))

    crop = flow_io.factor_crop if args.fit == "crop" else (lambda a: a)

    def load_pair(i):
        p0, p1, pf = pairs[i][:3]
        im0 = crop(np.asarray(Image.open(p0).convert("RGB")))
        im1 = crop(np.asarray(Image.open(p1).convert("RGB")))
        raw = flow_io.read_flo(pf)
        gt = crop(raw)
        valid = flow_io.flow_valid(gt)                        # the .flo sentinel
        if len(pairs[i]) > 3:
            mask = np.asarray(Image.open(pairs[i][3]).convert("L")) != 0
            if mask.shape != raw.shape[:2]:
                raise SystemExit(f"evaluate.py: mask {pairs[i][3]} is {mask.shape}, its flow {raw.shape[:2]}")
            valid &= crop((~mask if args.mask_is_invalid else mask)[..., None])[..., 0]
        if args.fit != "crop":                                    # uint8 frames: a quarter of the upload, / 255 in the fit launch
            if im0.shape != im1.shape or im0.shape[:2] != gt.shape[:2]:
                raise SystemExit(f"evaluate.py: pair {i}: frames {im0.shape[:2]}, {im1.shape[:2]} and flow {gt.shape[:2]} differ in size")
            return (torch.from_numpy(np.array(im0)), torch.from_numpy(np.array(im1)),          # (copies: PIL's buffers are read-only)
                    torch.from_numpy(np.ascontiguousarray(gt, np.float32)), torch.from_numpy(np.ascontiguousarray(valid)))
        return (torch.from_numpy(np.ascontiguousarray(im0, np.float32) / 255.0),
                torch.from_numpy(np.ascontiguousarray(im1, np.float32) / 255.0),
                torch.from_numpy(np.ascontiguousarray(gt, np.float32)),
                torch.from_numpy(np.ascontiguousarray(valid)))

    def forward(im0, im1):
        if args.fit != "crop":
            flow = pwcnet_amd.flow_any_size(model, im0, im1, args.fit)[0]
        else:
            flow = model(im0, im1)[0]
        if filt is not None:                                      # guided by the first frame on the flow's grid
            flow = pwcnet_amd.filter_flow(flow, guide=im0, **filt)[0]
        return flow

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = sharding.evaluate_pairs(forward, load_pair, len(pairs), args.batch, dist, dev, gather=args.save_dir is not None,
                                  metrics=True)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dist is None or dist.get_rank() == 0:
        if args.save_dir:
            os.makedirs(args.save_dir, exist_ok=True)
            for i, f in enumerate(res["flows"].cpu().numpy()):
                flow_io.write_flo(os.path.join(args.save_dir, f"{i:06d}.flo"), f)
            if args.save_vis:                                     # in batches: three pictures per index, only uint8 comes back
                for b0 in range(0, len(pairs), args.batch):
                    idx = range(b0, min(b0 + args.batch, len(pairs)))
                    loaded = [load_pair(i)[2:] for i in idx]
                    gt = torch.stack([g for g, _ in loaded]).to(dev)
                    valid = torch.stack([v for _, v in loaded]).to(dev)
                    pred = res["flows"][b0:b0 + len(idx)]
                    rad = pwcnet_amd.flow_max_radius(gt, valid)
                    pictures = {"": pwcnet_amd.flow_to_color(pred, rad), "_gt": pwcnet_amd.flow_to_color(gt, rad, valid),
                                "_err": pwcnet_amd.flow_error_color(pred, gt, valid)}
                    for tag, batch in pictures.items():
                        for i, picture in zip(idx, batch.cpu().numpy()):
                            Image.fromarray(picture).save(os.path.join(args.save_dir, f"{i:06d}{tag}.png"))
        out = {"epe": res["epe"], "pairs": res["pairs"], "seconds": dt, "n_gpus": world}
        out.update({k: res[k] for k in ("fl_all", "px1", "px3", "px5", "epe_s0_10", "epe_s10_40", "epe_s40", "valid_px")})
        out["per_pair_epe"] = res["per_pair_epe"]
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Counterpart of the reference's test.py (inference + timing CLI) on the HIP path.

    python infer.py --input_images frame_0.png frame_1.png [--resume model_600.ckpt] [--time]

Follows reference test.py:27-65: crop both images to multiples of 64 (--fit crop, the default; --fit resize / pad keep the
whole frame: it is resized or padded to the next multiples of 64 on the GPU and flow_final comes back on the frame's own grid,
the pyramid levels stay at the network's geometry), scale to [0,1],
batch of one pair, default PWCDCNet(), optional checkpoint restore (TF V2 bundle, read
without TensorFlow), optional timing loop over repeated forwards of the same pair, then
the 5-level flow pyramid rescaled to pixels at each level (x 20 / 2^(6-l), test.py:57-60).
Writes <out>/flow_final.flo plus a colour-coded PNG per pyramid level instead of the
reference's matplotlib PDF.  --vis gpu colours the PNGs on the GPU (pwcnet_amd.vis) instead of with numpy on copied-back flows;
the .flo does not depend on it.  No interactive GPU prompt: the device is cuda:<--gpu>.
--flow_filter R filters flow_final before it is written and coloured: the weighted median over a (2 R + 1)^2 window, R = 1 .. 7,
guided by the first frame at the flow's geometry (pwcnet_amd.filter_flow; after the refit where --fit is not crop), with
--flow_filter_sigma_space (pixels), --flow_filter_sigma_color (grey levels per channel) [a box, no colour term] and
--flow_filter_iters [1].  Untuned: nobody has measured what it does to the error.
"""
import argparse
import os
import time

import numpy as np
import torch


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--input_images", type=str, nargs=2, required=True, help="Target images (required)")
    ap.add_argument("--resume", type=str, default=None, help="Learned parameter checkpoint prefix [None]")
    ap.add_argument("--time", "-t", action="store_true", help="measure inference speed")
    ap.add_argument("--iters", type=int, default=1000, help="timed iterations with --time [1000]")
    ap.add_argument("--out", type=str, default="./test_figure")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--fit", choices=("crop", "resize", "pad"), default="crop",
                    help="frames whose size is no multiple of 64: crop them (reference), or resize / pad them on the GPU and "
                         "bring the flow back to the frame's size [crop]")
    ap.add_argument("--normalize_features", action="store_true",
                    help="correlate layer-normalised feature maps (PWCDCNet(normalize_features=True)).  A checkpoint carries no marker for this: pass it exactly when the weights were trained with it")
    ap.add_argument("--norm_eps", type=float, default=1e-16, help="--normalize_features: epsilon under the square root [1e-16]")
    ap.add_argument("--vis", choices=("host", "gpu"), default="host",
                    help="colour the PNGs with numpy on the copied-back flows, or on the GPU (pwcnet_amd.vis: only uint8 pictures "
                         "and the final flow cross to the host) [host]")
    from pwcnet_amd.flow_filter import add_cli_arguments
    add_cli_arguments(ap)
    return ap


def main():
    ap = build_parser()
    args = ap.parse_args()
    from pwcnet_amd.flow_filter import check_cli_arguments
    filt = check_cli_arguments(ap, args)                                   # filter_flow's keyword arguments, None without the flag

    from PIL import Image
    import pwcnet_amd
    from pwcnet_amd import ckpt, flow_io

    torch.cuda.set_device(args.gpu)
    if args.fit == "crop":
        imgs = [flow_io.factor_crop(np.asarray(Image.open(p).convert("RGB"))) for p in args.input_images]
        images = np.array(imgs, dtype=np.float32) / 255.0                  # (2, h, w, 3)
        x = torch.from_numpy(images).cuda()
        guide = x[0:1]                                                     # (u8 / 255 as float32 goes back to the same bytes)
    else:                                                                  # uint8 upload; / 255 and the fit in one launch
        x = torch.from_numpy(np.stack([np.asarray(Image.open(p).convert("RGB")) for p in args.input_images])).cuda()
        guide = x[0:1]                                                     # the first frame on its own grid, uint8
        x, info = pwcnet_amd.fit_frames(x, args.fit)

    model = pwcnet_amd.PWCDCNet(range_check="sync", normalize_features=args.normalize_features, norm_eps=args.norm_eps)      # results are final when a call returns (fp16-range check + fp32 repeat)
    if args.resume is not None:
        print(f"Loading learned model from checkpoint {args.resume}")
        model.load_weights(ckpt.load_weights(args.resume))
    else:
        print("!!! Test with un-learned model !!!")

    flow_final, flows = model(x[0:1], x[1:2])
    if args.time:
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(args.iters):
            flow_final, flows = model(x[0:1], x[1:2])
        torch.cuda.synchronize()
        print(f"Inference time: {(time.time() - t0) / args.iters} sec (averaged over {args.iters} iterations)")
    if args.fit != "crop":
        flow_final = pwcnet_amd.refit_flow(flow_final, info)               # the frame's own size, frame pixels
    if filt is not None:
        flow_final = pwcnet_amd.filter_flow(flow_final, guide=guide, **filt)[0]

    os.makedirs(args.out, exist_ok=True)
    flow_io.write_flo(os.path.join(args.out, "flow_final.flo"), flow_final[0].cpu().numpy())
    for l, flow in enumerate(flows):
        upscale = 20.0 / 2 ** (model.num_levels - l)
        if args.vis == "gpu":
            picture = pwcnet_amd.flow_to_color(flow[0:1], flow_scale=upscale)[0].cpu().numpy()
        else:
            picture = flow_io.flow_to_color(flow[0].cpu().numpy() * upscale)
        Image.fromarray(picture).save(os.path.join(args.out, f"flow_level{l}.png"))
    if args.vis == "gpu":
        picture = pwcnet_amd.flow_to_color(flow_final[0:1])[0].cpu().numpy()
    else:
        picture = flow_io.flow_to_color(flow_final[0].cpu().numpy())
    Image.fromarray(picture).save(os.path.join(args.out, "flow_final.png"))
    print("Figure saved")


if __name__ == "__main__":
    main()

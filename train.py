#!/usr/bin/env python
"""Counterpart of the reference's train.py on the HIP path (pwcnet_amd.train.Trainer).

    python train.py -dd <dataset_dir> [-e 100] [-b 4] [--crop_shape 384 448] [--lr 1e-4] [--gamma 4e-4] ...
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py -dd <dir> ...

Follows reference train.py:110-170: per epoch a pass over the training pairs (images / 255, un-scaled ground-truth
flow), one Adam step per batch, then validation (EPE of flows_final, train.py:77), then `./model/model_<epoch>.ckpt`
-- written as a TensorFlow V2 bundle (pwcnet_amd.ckpt, no TensorFlow needed) that the reference's Saver and this
repo's infer.py can restore.  Same argument names and defaults as the reference where they apply; no interactive
GPU prompt (one process per GPU, LOCAL_RANK picks the device; gradients are averaged with one RCCL all-reduce).

Dataset: the reference's loaders live in its empty `datahandler` submodule; here a directory is scanned for
MPI-Sintel-style pairs  <dir>/<pass>/<seq>/frame_NNNN.png  with  <dir>/flow/<seq>/frame_NNNN.flo , or, with
`--dataset synthetic`, random translating textures with known flow are generated (no files needed).
Both use_dc settings and both losses (multiscale, robust) are implemented (Trainer docstring).

`--loss unsup` trains without labels: PWCDCNetModule under torch.optim.Adam on photometric_loss(flows_final) + --smooth_weight *
smoothness_loss(flows_final, images_0) (pwcnet_amd/unsup.py: images_1 warped by the predicted flow against images_0, and an
edge-aware first-order smoothness of the flow).  Ground truth, where the data set has it, is used for the validation line only.
`--photo census` replaces the data term by census_loss(flows_final, radius=--census_radius): the soft census (ternary) term on the
local intensity order, which a brightness change between the frames does not move.
`--ssim_weight W` (0 <= W <= 1) blends the SSIM term into the data term: (1 - W) * <the --photo term> + W * ssim_loss(flows_final,
radius=--ssim_radius), (1 - SSIM) / 2 per channel over the (2r+1)^2 windows every pixel of which is in frame -- in both directions and
under the masks with --occlusion fb.  The step line then prints `ssim <value>` after the base term's value; W = 1 computes and
prints no base term, W = 0 (the default) no SSIM: the run as it was.  `--photo charbonnier --ssim_weight 0.85` is ARFlow's
first-stage data term (0.15 L1 + 0.85 SSIM, 3 x 3 windows); UFlow and ARFlow's second stage add the census term.
`--occlusion fb` leaves occluded pixels out of the data term: ONE module forward on the pairs in both orders stacked along the
batch axis (batch 2N) gives the forward and the backward flow, fb_valid (pwcnet_amd/unsup.py; --occ_alpha1, --occ_alpha2, UnFlow's
forward-backward check) turns them into two masks -- constants, no gradient goes through them -- and the loss is the data term
in both directions, each under its mask, plus --smooth_weight * the smoothness of both flows, each against its own first image,
the total halved so that --smooth_weight keeps its meaning.  The step line then also prints the occluded fraction.  Validation
is unchanged (forward flow only).
`--smooth_order 2` penalises the second difference of the flow instead of the first (smoothness_loss(order=2): a constant slope
is free), and `--consistency_weight W` (with --occlusion fb) adds W * fb_consistency_loss(fw, bw) under the two masks: UnFlow's
third term, rho of the forward flow plus the backward flow sampled where it points to, with gradients into both flows; the step
line then ends in `consistency <value>`.  Together with --photo census this is UnFlow's loss.
`--occlusion range` is the same stacked 2N forward with range-map masks in place of the forward-backward check (Wang et al. 2018,
UFlow's default for Chairs and Sintel): range_valid (pwcnet_amd/splat.py) splats a 1 from every pixel of frame 1 along the backward
flow, and a frame-0 pixel is kept when at least --occ_min_range (0.5: a choice, nobody has trained with it yet) lands on it; the
backward mask likewise from the forward flow.  The check of fb cannot tell "occluded" from "the flow is still wrong" and masks
out most of the frame early in training; the range map of a poor flow still covers most of it.  The occluded fraction on the step
line is counted from the masks, and --consistency_weight goes with either mode.
`--level_weights W0 W1 W2 W3 W4` (one weight per flows_pyramid entry, coarse -> fine: 1/64 .. 1/4 of the frame) puts the loss on every
pyramid level as well, as UnFlow, DDFlow and ARFlow train PWC-Net: frame_pyramid (pwcnet_amd/pyramid.py, one launch per frame
batch, on what the step holds after --augment) gives the block means of both frames at the five sizes, and the step adds
sum_l W_l * (data term at level l + --smooth_weight * smoothness at level l) -- the same data, SSIM and smoothness terms on the
level frames and flows_pyramid[l], with flow_scale = level_flow_scale (20 / 2^level: the level's own pixels; the smoothness terms
take the flow already multiplied by it).  With --occlusion fb | range both directions are added and halved as above, under
mask_pyramid of the two masks: a level pixel is kept when at least --occ_pool (0.5: a choice, nobody has trained with it yet) of
its block is.  The consistency term stays on flows_final.  The step line then ends in `levels <v0> <v1> <v2> <v3> <v4>`, the
unweighted data value of each level; a level too small for a term (a window of --census_radius 3 on a 1 x 2 level) prints nan and
adds nothing.  Absent or all zeros: the run as it was, no pyramid launch, the same step lines.
`--selfsup_weight W` adds the self-supervision term of DDFlow, SelFlow, UFlow and ARFlow: after the step's forward and backward at
--crop_shape, the same network runs on the centre window of the same frames (--selfsup_crop C pixels removed per side, cut on the
GPU by augment_pairs(crop_params(N, C, C)), the plain crop), and W * flow_distill_loss (pwcnet_amd/unsup.py) pulls that student
flow to the first pass's detached flow read through the window: a pixel that leaves the narrow frame has no photometric signal
there, and the wide pass often still sees where it goes.  The wide pass is the one that is trained and the teacher (UFlow's
arrangement): two forwards and two backwards per step, one optimiser step.  --selfsup_mask occluded (the default with --occlusion
fb | range) takes the pixels where the wide pass's occlusion check passed and the student's own check, with the same settings,
failed; teacher: where the wide pass's passed; all (the default without occlusion): every pixel.  --selfsup_after K starts the term
and its forward at global step K.  The step line then ends in `selfsup <value>  selfsup_share <the share of the student pixels
that contributed>`, and loss/unsup includes W * the term.  W = 0 (the default): the step as it was, no second forward.
Single process, constant learning rate; --gamma is Adam's weight_decay (the same gamma * l2_loss gradient).

Sparse ground truth: every pair comes with a validity mask -- the .flo "unknown" sentinel (|u| or |v| above 1e9),
and-ed with <dir>/invalid/<seq>/frame_NNNN.png (non-zero = invalid, MPI-Sintel's layout) where that file exists -- and
the step's loss and gradient and the validation numbers (masked EPE, KITTI's Fl-all) leave the invalid pixels out.
`--synthetic_invalid F` knocks a random fraction F of the synthetic ground truth out and writes 1e10 there.  KITTI's
16-bit flow PNGs are not read: convert them to .flo (sentinel at the unlabelled pixels) first.

`--augment geometric | full` prepares the training batches on the GPU (pwcnet_amd/augment.py, one launch per batch): the data set
hands back WHOLE uint8 frames, flow and mask, the batch is uploaded as bytes, and every pair gets its own random zoom
(--aug_scale), rotation (--aug_rotate), translation (--aug_translate), mirror (--aug_flip) and a small extra rotation and shift
of the second frame (--aug_rel_rotate, --aug_rel_translate), the ground-truth flow transformed with them; `full` adds gain, gamma,
contrast and brightness jitter.  The crop stays --crop_shape; --aug_seed seeds the draws.  The frames of a batch must have one
size.  `--dataset synthetic` then generates its frames 32 px larger on each side than the crop.  Validation is untouched: it runs
on the plain crops.  `--augment none` (the default) is the data path as it was: the host crop, / 255, the float32 upload.
"""
import argparse
import glob
import os
import time

import numpy as np
import torch


def sintel_pairs(root, render="clean"):
    pairs = []
    for seq in sorted(glob.glob(os.path.join(root, render, "*"))):
        frames = sorted(glob.glob(os.path.join(seq, "frame_*.png")))
        for a, b in zip(frames[:-1], frames[1:]):
            flo = os.path.join(root, "flow", os.path.basename(seq), os.path.basename(a).replace(".png", ".flo"))
            if os.path.exists(flo):
                pairs.append((a, b, flo))
    return pairs


class SyntheticPairs:
    """Random smooth textures translated by a per-pair integer shift; ground truth = that shift.  invalid: the fraction of
    the pixels (a seeded random set per pair) whose label is knocked out: mask False and ground truth 1e10, the .flo
    sentinel, so that a consumer that ignored the mask would show it at once."""

    def __init__(self, n, shape, seed=0, invalid=0.0, uint8=False):
        self.n, self.shape, self.seed, self.invalid = n, shape, seed, float(invalid)
        self.uint8 = uint8                      # frames rounded to bytes, as files hold them (--augment uploads bytes)

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        rng = np.random.RandomState(self.seed + i)
        h, w = self.shape
        sx, sy = rng.randint(-6, 7), rng.randint(-6, 7)
        base = rng.uniform(0, 255, size=(h // 8 + 4, w // 8 + 4, 3)).astype(np.float32)
        big = np.kron(base, np.ones((8, 8, 1), np.float32))
        im0 = big[16:16 + h, 16:16 + w]
        im1 = big[16 - sy:16 - sy + h, 16 - sx:16 - sx + w]       # im1(p) = im0(p - s): content moves by +s
        flow = np.empty((h, w, 2), np.float32)
        flow[..., 0], flow[..., 1] = sx, sy
        valid = np.ones((h, w), bool)
        if self.invalid > 0:
            valid = np.random.RandomState(self.seed + 7919 * (i + 1)).uniform(size=(h, w)) >= self.invalid
            flow[~valid] = 1e10
        if self.uint8:
            im0, im1 = np.rint(im0).astype(np.uint8), np.rint(im1).astype(np.uint8)
        return np.ascontiguousarray(im0), np.ascontiguousarray(im1), flow, valid


class FilePairs:
    def __init__(self, pairs, crop_shape, crop_type="random", seed=0, whole=False):
        self.pairs, self.crop, self.crop_type = pairs, crop_shape, crop_type
        self.rng = np.random.RandomState(seed)
        self.whole = whole                      # --augment: whole uint8 frames, flow and mask; the crop happens on the GPU

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, i):
        from PIL import Image
        from pwcnet_amd import flow_io
        a, b, f = self.pairs[i]
        im0, im1 = (np.asarray(Image.open(p).convert("RGB"), np.uint8 if self.whole else np.float32) for p in (a, b))
        flow = flow_io.read_flo(f)
        valid = flow_io.flow_valid(flow)
        inv = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(f))), "invalid",
                           os.path.basename(os.path.dirname(f)), os.path.basename(f).replace(".flo", ".png"))
        if os.path.exists(inv):
            valid &= np.asarray(Image.open(inv).convert("L")) == 0
        if self.whole:
            return np.ascontiguousarray(im0), np.ascontiguousarray(im1), np.ascontiguousarray(flow), np.ascontiguousarray(valid)
        ch, cw = self.crop
        H, W = im0.shape[:2]
        y0 = self.rng.randint(0, H - ch + 1) if self.crop_type == "random" else (H - ch) // 2
        x0 = self.rng.randint(0, W - cw + 1) if self.crop_type == "random" else (W - cw) // 2
        sl = (slice(y0, y0 + ch), slice(x0, x0 + cw))
        return (np.ascontiguousarray(im0[sl]), np.ascontiguousarray(im1[sl]), np.ascontiguousarray(flow[sl]),
                np.ascontiguousarray(valid[sl]))


def batches(ds, idx, bs, same_size=False):
    for i in range(0, len(idx) - bs + 1, bs):                       # drop_last, like the reference's loader
        items = [ds[j] for j in idx[i:i + bs]]
        if same_size and len({it[0].shape for it in items}) > 1:    # whole frames (--augment): one launch takes one frame size
            raise ValueError(f"train.py --augment: the frames of a batch differ in size, {sorted({it[0].shape[:2] for it in items})}; "
                             "use a data set of one frame size or --batch_size 1")
        yield tuple(torch.from_numpy(np.stack([it[k] for it in items])) for k in range(4))


class Augmenter:
    """--augment: one record per pair from draw_params (seeded: --aug_seed + rank), one augment_pairs launch per batch.  Takes the
    host batch of whole frames as batches() yields it and returns (images_0, images_1, flows_gt, valid) on the GPU: float32
    frames in [0, 1] at --crop_shape, the transformed flow and its mask (None, None without flows)."""

    def __init__(self, args, rank=0):
        self.crop = tuple(args.crop_shape)
        self.rng = np.random.RandomState(args.aug_seed + rank)
        self.kw = dict(scale=tuple(args.aug_scale), rotate_deg=args.aug_rotate, translate_frac=args.aug_translate, flip=args.aug_flip,
                       rel_rotate_deg=args.aug_rel_rotate, rel_translate_px=args.aug_rel_translate, color=args.augment == "full")

    def __call__(self, images_0, images_1, flows=None, valid=None):
        from pwcnet_amd import augment_pairs, draw_params
        N, H, W, _ = images_0.shape
        params = draw_params(N, (H, W), self.crop, self.rng, **self.kw)
        if flows is not None:
            flows = flows.cuda()
            valid = None if valid is None or bool(valid.all()) else valid.cuda()
        return augment_pairs(images_0.cuda(), images_1.cuda(), params, self.crop, flows=flows, valid=valid)


def validate(args, weights, ds, val_idx, dist=None):
    """EPE / Fl-all of flows_final over the validation pairs (reference train.py:77,124-131), sharded over the ranks."""
    from pwcnet_amd import PWCDCNet, sharding
    net = PWCDCNet(num_levels=args.num_levels, search_range=args.search_range, warp_type=args.warp_type,
                   use_dc=args.use_dc, output_level=args.output_level, normalize_features=args.normalize_features,
                   norm_eps=args.norm_eps)
    net.load_weights(weights)
    return sharding.evaluate_pairs(lambda a, b: net(a / 255.0, b / 255.0)[0],
                                   lambda i: tuple(torch.from_numpy(x) for x in ds[val_idx[i]]),
                                   len(val_idx), batch=args.batch_size, dist=dist, device="cuda", metrics=True)


def unsup_step(model, objective, images_0, images_1, selfsup_weight=0.0, selfsup_crop=64):
    """The forwards and backwards of one label-free step (the caller zeroes the gradients before and steps the optimiser after):
    (loss, terms), both detached.  selfsup_weight > 0 adds the self-supervision pass; 0 is the step without it, launch for launch."""
    stacked = objective.occlusion != "none"
    if stacked:
        # both pair orders in one forward: the first N flows are 0 -> 1, the last N are 1 -> 0
        flows_final, flows_pyramid = model(torch.cat([images_0, images_1]), torch.cat([images_1, images_0]))
    else:
        flows_final, flows_pyramid = model(images_0, images_1)
    N, H, W, _ = images_0.shape
    teacher_masks = None
    if selfsup_weight > 0 and objective.selfsup_mask != "all":
        # the wide pass is also the teacher: its masks are made here once and handed to the objective
        teacher_masks = objective.masks(flows_final[:N], flows_final[N:])[:2]
    loss, terms = objective(images_0, images_1, flows_final, flows_pyramid, masks=teacher_masks)
    loss.backward()
    if not selfsup_weight > 0:
        return loss.detach(), terms
    # the first tape is spent (one tape of the module alive at a time).  The student is the same network on the centre window of
    # the same frames; its flow is pulled to the wide pass's, read through the window, where that one saw more
    from pwcnet_amd import augment_pairs, crop_params
    C = selfsup_crop
    teacher, loss = flows_final.detach(), loss.detach()
    del flows_final, flows_pyramid
    small_0, small_1, _, _ = augment_pairs(images_0, images_1, crop_params(N, C, C), (H - 2 * C, W - 2 * C))
    if stacked:
        student, _ = model(torch.cat([small_0, small_1]), torch.cat([small_1, small_0]))
    else:
        student, _ = model(small_0, small_1)
    student_masks = None
    if objective.selfsup_mask == "occluded":
        student_masks = objective.masks(student[:N], student[N:])[:2]
    term, counts = objective.selfsup_term(student, teacher, (C, C), teacher_masks, student_masks, return_counts=True)
    (selfsup_weight * term).backward()
    terms["selfsup"] = term.detach()
    terms["selfsup_share"] = float(counts.sum()) / float(student.shape[0] * student.shape[1] * student.shape[2])
    return loss + selfsup_weight * term.detach(), terms


def train_unsup(args, ds, train_idx, val_idx, val_ds=None, aug=None):
    """--loss unsup: no ground truth reaches the step; checkpoints through tf_state_dict(), so they load into PWCDCNet.
    aug (an Augmenter, --augment): `ds` holds whole frames, the batch is cut and jittered on the GPU, validation reads val_ds."""
    from pwcnet_amd import PWCDCNetModule, UnsupObjective, ckpt
    objective = UnsupObjective(photo=args.photo, census_radius=args.census_radius, photo_eps=args.photo_eps, photo_q=args.photo_q,
                               ssim_weight=args.ssim_weight, ssim_radius=args.ssim_radius, smooth_weight=args.smooth_weight,
                               smooth_order=args.smooth_order, edge_alpha=args.edge_alpha, occlusion=args.occlusion,
                               occ_alpha1=args.occ_alpha1, occ_alpha2=args.occ_alpha2, occ_min_range=args.occ_min_range,
                               consistency_weight=args.consistency_weight, level_weights=args.level_weights,
                               occ_pool=args.occ_pool, selfsup_mask=args.selfsup_mask)

    model = PWCDCNetModule(num_levels=args.num_levels, search_range=args.search_range, warp_type=args.warp_type,
                           use_dc=args.use_dc, output_level=args.output_level, normalize_features=args.normalize_features,
                           norm_eps=args.norm_eps)
    if args.resume is not None:
        print(f"Loading learned model from checkpoint {args.resume}")
        model.load_weights(ckpt.load_weights(args.resume))
    opt = torch.optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.gamma)
    global_step = 0
    for e in range(args.num_epochs):
        order = np.random.RandomState(1000 + e).permutation(train_idx)
        steps = len(order) // args.batch_size
        t0, loss_sum, n_steps = time.time(), 0.0, 0
        for images_0, images_1, _, _ in batches(ds, order[:steps * args.batch_size], args.batch_size, same_size=aug is not None):
            if aug is not None:
                images_0, images_1, _, _ = aug(images_0, images_1)
            else:
                images_0, images_1 = (images_0 / 255.0).cuda(), (images_1 / 255.0).cuda()
            opt.zero_grad(set_to_none=True)
            selfsup = args.selfsup_weight if global_step + 1 >= args.selfsup_after else 0.0
            loss, terms = unsup_step(model, objective, images_0, images_1, selfsup, args.selfsup_crop)
            opt.step()
            global_step += 1
            n_steps += 1
            loss_sum += float(loss)
            line = "".join(f"  {k} {float(terms[k]):.6f}" for k in (objective.term, "ssim", "smoothness") if k in terms)
            if "occluded" in terms:
                line += f"  occluded {terms['occluded']:.4f}"
            if "consistency" in terms:
                line += f"  consistency {float(terms['consistency']):.6f}"
            if "levels" in terms:
                line += "  levels " + " ".join(f"{v:.6f}" for v in terms["levels"])
            if "selfsup" in terms:
                line += f"  selfsup {float(terms['selfsup']):.6f}  selfsup_share {terms['selfsup_share']:.4f}"
            print(f"step {global_step}: loss/unsup {float(loss):.6f}{line}")
        res = validate(args, model.tf_state_dict(), ds if val_ds is None else val_ds, val_idx)
        dt = time.time() - t0
        print(f"epoch {e + 1}: loss/unsup {loss_sum / max(n_steps, 1):.4f}  EPE/val {res['epe']:.4f}  "
              f"Fl-all/val {res['fl_all']:.4f}  "
              f"global_step {global_step}  {n_steps * args.batch_size / max(dt, 1e-9):.1f} pairs/s")
        os.makedirs(args.model_dir, exist_ok=True)
        ckpt.save_weights(os.path.join(args.model_dir, f"model_{e + 1}.ckpt"), model.tf_state_dict())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-d", "--dataset", type=str, default="SintelClean", help="SintelClean | SintelFinal | synthetic")
    ap.add_argument("-dd", "--dataset_dir", type=str, default=None, help="Directory containing target dataset")
    ap.add_argument("-e", "--num_epochs", type=int, default=100, help="# of epochs [100]")
    ap.add_argument("-b", "--batch_size", type=int, default=4, help="Batch size per GPU [4]")
    ap.add_argument("--crop_type", type=str, default="random", help="Crop type for raw data [random]")
    ap.add_argument("--crop_shape", nargs=2, type=int, default=[384, 448], help="Crop shape for raw data [384, 448]")
    ap.add_argument("--num_levels", type=int, default=6)
    ap.add_argument("--search_range", type=int, default=4)
    ap.add_argument("--warp_type", default="bilinear", choices=["bilinear", "nearest"])
    ap.add_argument("--use-dc", dest="use_dc", action="store_true")
    ap.add_argument("--no-dc", dest="use_dc", action="store_false")
    ap.set_defaults(use_dc=False)
    ap.add_argument("--output_level", type=int, default=4)
    ap.add_argument("--normalize_features", action="store_true",
                    help="correlate layer-normalised feature maps: one norm over the two maps of a pair at every level, the "
                         "estimator keeps the raw ones.  A checkpoint carries no marker for this: infer.py, infer_continuous.py "
                         "and evaluate.py must be given the flag the weights were trained with")
    ap.add_argument("--norm_eps", type=float, default=1e-16, help="--normalize_features: epsilon under the square root [1e-16]")
    ap.add_argument("--loss", default="multiscale", choices=["multiscale", "robust", "unsup"],
                    help="multiscale | robust: supervised (Trainer); unsup: photometric + smoothness, no labels [multiscale]")
    ap.add_argument("--photo", default="charbonnier", choices=["charbonnier", "census"],
                    help="--loss unsup: the data term, Charbonnier on intensities or soft census on their local order [charbonnier]")
    ap.add_argument("--census_radius", type=int, default=3, choices=[1, 2, 3],
                    help="--photo census: window radius, (2r+1)^2 - 1 neighbours [3]")
    ap.add_argument("--ssim_weight", type=float, default=0.0, metavar="W",
                    help="--loss unsup: the data term becomes (1 - W) * <the --photo term> + W * SSIM term, W in [0, 1]; "
                         "--photo charbonnier --ssim_weight 0.85 is ARFlow's 0.15 L1 + 0.85 SSIM [0]")
    ap.add_argument("--ssim_radius", type=int, default=1, choices=[1, 2, 3],
                    help="--ssim_weight: window radius, (2r+1)^2 pixels; 1 is the 3 x 3 window of UFlow / ARFlow [1]")
    ap.add_argument("--occlusion", default="none", choices=["none", "fb", "range"], metavar="{none,fb}|range",
                    help="--loss unsup: none, or fb: forward-backward consistency masks on the data term, both directions "
                         "trained from one forward at batch 2N; range: the same forward, range-map masks (a pixel is kept when "
                         "enough of the other frame lands on it under the opposite flow) [none]")
    ap.add_argument("--occ_min_range", type=float, default=0.5,
                    help="--occlusion range: a pixel is kept when its range map is at least this [0.5]")
    ap.add_argument("--occ_alpha1", type=float, default=0.01,
                    help="--occlusion fb: |f + g|^2 <= alpha1 (|f|^2 + |g|^2) + alpha2 keeps a pixel [0.01]")
    ap.add_argument("--occ_alpha2", type=float, default=0.5, help="--occlusion fb: alpha2 of that check, px^2 [0.5]")
    ap.add_argument("--smooth_weight", type=float, default=0.1, help="--loss unsup: weight of the smoothness term [0.1]")
    ap.add_argument("--smooth_order", type=int, default=1, choices=[1, 2],
                    help="--loss unsup: the smoothness term penalises the first or the second difference of the flow [1]")
    ap.add_argument("--consistency_weight", type=float, default=0.0,
                    help="--occlusion fb: weight of the forward-backward consistency term, gradients into both flows [0]")
    ap.add_argument("--level_weights", nargs=5, type=float, default=None, metavar=("W0", "W1", "W2", "W3", "W4"),
                    help="--loss unsup: the data and smoothness terms on every flows_pyramid level as well, one weight per level, "
                         "coarse -> fine (1/64 .. 1/4 of the frame), on block-mean frame pyramids; absent or all zeros: the "
                         "loss on flows_final alone [absent]")
    ap.add_argument("--occ_pool", type=float, default=0.5, metavar="F",
                    help="--level_weights with --occlusion: a level pixel is kept when at least this fraction of its block "
                         "is, in (0, 1]; 1 is a min-pool (0.5 is a choice, nobody has trained with it yet) [0.5]")
    ap.add_argument("--selfsup_weight", type=float, default=0.0, metavar="W",
                    help="--loss unsup: weight of the self-supervision term -- a second forward on the centre window of the "
                         "batch, its flow against the first forward's through the window; 0: no second forward [0]")
    ap.add_argument("--selfsup_crop", type=int, default=64, metavar="C",
                    help="--selfsup_weight: pixels removed per side for the student view; --crop_shape - 2 C must be a "
                         "positive multiple of 64 in both axes [64]")
    ap.add_argument("--selfsup_after", type=int, default=0, metavar="K",
                    help="--selfsup_weight: the term and its forward start at global step K [0]")
    ap.add_argument("--selfsup_mask", default=None, choices=["occluded", "teacher", "all"],
                    help="--selfsup_weight: the pixels of the term -- occluded: the wide pass's occlusion check passed and the "
                         "student's failed (UFlow); teacher: the wide pass's passed; all: every pixel "
                         "[occluded with --occlusion fb | range, else all]")
    ap.add_argument("--photo_eps", type=float, default=1e-3, help="--loss unsup: Charbonnier epsilon of both terms [1e-3]")
    ap.add_argument("--photo_q", type=float, default=0.5, help="--loss unsup: Charbonnier exponent of both terms [0.5]")
    ap.add_argument("--edge_alpha", type=float, default=10.0,
                    help="--loss unsup: edge weight exp(-alpha * mean |image difference|) of the smoothness term [10]")
    ap.add_argument("--lr", type=float, default=1e-4, help="Learning rate [1e-4]")
    ap.add_argument("--lr_scheduling", dest="lr_scheduling", action="store_true")
    ap.add_argument("--no-lr_scheduling", dest="lr_scheduling", action="store_false")
    ap.set_defaults(lr_scheduling=True)
    ap.add_argument("--epsilon", type=float, default=0.02, help="robust loss epsilon [0.02]")
    ap.add_argument("--q", type=float, default=0.4, help="robust loss exponent [0.4]")
    ap.add_argument("--weights", nargs="+", type=float, default=[0.32, 0.08, 0.02, 0.01, 0.005])
    ap.add_argument("--gamma", type=float, default=0.0004, help="Coefficient for weight decay [4e-4]")
    ap.add_argument("-r", "--resume", type=str, default=None, help="Learned parameter checkpoint prefix [None]")
    ap.add_argument("--synthetic_pairs", type=int, default=64, help="pairs per epoch with --dataset synthetic")
    ap.add_argument("--synthetic_invalid", type=float, default=0.0,
                    help="fraction of the synthetic ground truth knocked out (mask False, flow 1e10) [0]")
    ap.add_argument("--augment", default="none", choices=["none", "geometric", "full"],
                    help="training batches prepared on the GPU from whole uint8 frames: geometric = random zoom, rotation, "
                         "translation, mirror and a small relative transform of the second frame, the flow transformed with them; "
                         "full = that and colour jitter; none = the host crop [none]")
    ap.add_argument("--aug_scale", nargs=2, type=float, default=[0.9, 1.3], metavar=("LO", "HI"), help="--augment: zoom range [0.9 1.3]")
    ap.add_argument("--aug_rotate", type=float, default=10.0, metavar="DEG", help="--augment: rotation within +-DEG [10]")
    ap.add_argument("--aug_translate", type=float, default=0.1, metavar="FRAC",
                    help="--augment: the crop's centre moves within +-FRAC of the frame's width and height [0.1]")
    ap.add_argument("--aug_flip", type=float, default=0.5, metavar="P", help="--augment: probability of a left-right mirror [0.5]")
    ap.add_argument("--aug_rel_rotate", type=float, default=1.0, metavar="DEG",
                    help="--augment: extra rotation of the second frame within +-DEG [1]")
    ap.add_argument("--aug_rel_translate", type=float, default=2.0, metavar="PX",
                    help="--augment: extra shift of the second frame within +-PX pixels [2]")
    ap.add_argument("--aug_seed", type=int, default=0, help="--augment: seed of the draws (+ rank) [0]")
    ap.add_argument("--val_fraction", type=float, default=0.1)
    ap.add_argument("--model_dir", type=str, default="./model")
    args = ap.parse_args()
    # what the training path does not build is refused here, not by an assert after the data set has been read
    if args.warp_type != "bilinear":
        ap.error("--warp_type nearest has no gradient path here (the reference trains with its model default, bilinear)")
    if args.num_levels != 6 or args.search_range != 4:
        ap.error("training supports --num_levels 6 --search_range 4 (the reference's scales and *20 hard-code 6 levels)")
    if not 0 <= args.output_level < args.num_levels:
        ap.error("--output_level must be in [0, num_levels)")
    if not 0.0 <= args.synthetic_invalid < 1.0:
        ap.error("--synthetic_invalid must be in [0, 1)")
    if args.occlusion != "none" and args.loss != "unsup":
        ap.error(f"--occlusion {args.occlusion} belongs to --loss unsup (the supervised losses have ground truth and its own mask)")
    if not (args.occ_alpha1 >= 0 and args.occ_alpha2 >= 0):
        ap.error("--occ_alpha1 and --occ_alpha2 must be non-negative")
    if not args.occ_min_range >= 0:
        ap.error("--occ_min_range must be non-negative")
    if not args.consistency_weight >= 0:
        ap.error("--consistency_weight must be non-negative")
    if args.consistency_weight > 0 and args.occlusion == "none":
        ap.error("--consistency_weight needs --occlusion fb or range (the term reads the forward and the backward flow of one "
                 "forward)")
    if not 0.0 <= args.ssim_weight <= 1.0:
        ap.error("--ssim_weight must be in [0, 1]")
    if args.ssim_weight > 0 and args.loss != "unsup":
        ap.error("--ssim_weight belongs to --loss unsup")
    if args.smooth_order != 1 and args.loss != "unsup":
        ap.error("--smooth_order belongs to --loss unsup")
    if args.level_weights is not None:
        if args.loss != "unsup":
            ap.error("--level_weights belongs to --loss unsup (the supervised losses weigh the levels with --weights)")
        if min(args.level_weights) < 0:
            ap.error("--level_weights must be non-negative")
        if args.output_level != 4:
            ap.error("--level_weights takes one weight per flows_pyramid entry: five, with --output_level 4")
    if not 0.0 < args.occ_pool <= 1.0:
        ap.error("--occ_pool must be in (0, 1]")
    if not args.selfsup_weight >= 0:
        ap.error("--selfsup_weight must be non-negative")
    if args.selfsup_weight > 0 and args.loss != "unsup":
        ap.error("--selfsup_weight belongs to --loss unsup")
    if args.selfsup_crop <= 0:
        ap.error("--selfsup_crop must be positive (the student view is narrower than the batch's)")
    if args.selfsup_after < 0:
        ap.error("--selfsup_after must be non-negative")
    if args.selfsup_weight > 0 and any(v - 2 * args.selfsup_crop < 64 or (v - 2 * args.selfsup_crop) % 64 for v in args.crop_shape):
        ap.error(f"--selfsup_crop {args.selfsup_crop}: --crop_shape minus twice the crop must be a positive multiple of 64 in both "
                 f"axes (the student view goes through the network), got "
                 f"{args.crop_shape[0] - 2 * args.selfsup_crop} x {args.crop_shape[1] - 2 * args.selfsup_crop}")
    if args.selfsup_mask in ("occluded", "teacher") and args.occlusion == "none":
        ap.error(f"--selfsup_mask {args.selfsup_mask} reads the occlusion masks: it needs --occlusion fb or range")
    if not 0 < args.aug_scale[0] <= args.aug_scale[1]:
        ap.error("--aug_scale LO HI must satisfy 0 < LO <= HI")
    if min(args.aug_rotate, args.aug_translate, args.aug_rel_rotate, args.aug_rel_translate) < 0 or not 0 <= args.aug_flip <= 1:
        ap.error("--aug_rotate, --aug_translate, --aug_rel_rotate, --aug_rel_translate must be non-negative, --aug_flip in [0, 1]")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.loss == "unsup":
        if world > 1:
            raise SystemExit("train.py: --loss unsup runs in a single process (no multi-GPU label-free training): "
                             f"launched with WORLD_SIZE={world}")
        if args.output_level not in (4, 5):
            ap.error("--loss unsup: --output_level 4 or 5 (PWCDCNetModule's gradient of the final resize)")
        if not (args.photo_eps > 0 and 0 < args.photo_q <= 1 and args.edge_alpha >= 0):
            ap.error("--photo_eps must be positive, --photo_q in (0, 1], --edge_alpha non-negative")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    if rank == 0:
        for key, item in vars(args).items():
            print(f"{key} : {item}")

    from pwcnet_amd import ckpt, sharding
    from pwcnet_amd.train import Trainer

    if args.dataset == "synthetic":
        ds = SyntheticPairs(args.synthetic_pairs, tuple(args.crop_shape), invalid=args.synthetic_invalid)
    else:
        if not args.dataset_dir:
            raise SystemExit("train.py: --dataset_dir is required for file datasets")
        pairs = sintel_pairs(args.dataset_dir, "final" if args.dataset == "SintelFinal" else "clean")
        if not pairs:
            raise SystemExit(f"train.py: no frame pairs with flow found under {args.dataset_dir}")
        ds = FilePairs(pairs, tuple(args.crop_shape), args.crop_type)
    aug = val_ds = None
    if args.augment != "none":
        # training reads whole uint8 frames and cuts them on the GPU; validation keeps the data set above
        aug, val_ds = Augmenter(args, rank), ds
        if args.dataset == "synthetic":
            ds = SyntheticPairs(args.synthetic_pairs, (args.crop_shape[0] + 64, args.crop_shape[1] + 64),
                                invalid=args.synthetic_invalid, uint8=True)
        else:
            ds = FilePairs(pairs, tuple(args.crop_shape), args.crop_type, whole=True)
    n_val = max(1, int(len(ds) * args.val_fraction))
    perm = np.random.RandomState(0).permutation(len(ds))
    val_idx, train_idx = perm[:n_val], perm[n_val:]
    if args.loss == "unsup":
        return train_unsup(args, ds, train_idx, val_idx, val_ds, aug)

    trainer = Trainer(num_levels=args.num_levels, search_range=args.search_range, warp_type=args.warp_type,
                      use_dc=args.use_dc, output_level=args.output_level, weights=args.weights, gamma=args.gamma,
                      lr=args.lr, lr_scheduling=args.lr_scheduling, device=f"cuda:{local_rank}", dist=dist,
                      loss=args.loss, epsilon=args.epsilon, q=args.q, normalize_features=args.normalize_features,
                      norm_eps=args.norm_eps)
    if args.resume is not None:
        print(f"Loading learned model from checkpoint {args.resume}")
        trainer.load_weights(ckpt.load_weights(args.resume))

    for e in range(args.num_epochs):
        order = np.random.RandomState(1000 + e).permutation(train_idx)
        lo, hi = sharding.shard_range(len(order), world, rank)       # pairs shard across the ranks
        steps = (hi - lo) // args.batch_size
        if dist is not None:                                          # every rank must take the same number of steps
            st = torch.tensor([steps], device="cuda")
            dist.all_reduce(st, op=dist.ReduceOp.MIN)
            steps = int(st.item())
        t0, loss_sum, n_steps = time.time(), 0.0, 0
        for images_0, images_1, flows_gt, valid in batches(ds, order[lo:lo + steps * args.batch_size], args.batch_size,
                                                           same_size=aug is not None):
            # a dense batch takes the step without a mask (the same kernels as before masks existed)
            if aug is not None:
                images_0, images_1, flows_gt, valid = aug(images_0, images_1, flows_gt, valid)
                loss = trainer.step(images_0, images_1, flows_gt, None if bool(valid.all()) else valid)
            else:
                loss = trainer.step((images_0 / 255.0).cuda(), (images_1 / 255.0).cuda(), flows_gt.cuda(),
                                    None if bool(valid.all()) else valid.cuda())
            loss_sum += float(loss)
            n_steps += 1
        res = validate(args, trainer.state_dict(), ds if val_ds is None else val_ds, val_idx, dist)
        if rank == 0:
            dt = time.time() - t0
            print(f"epoch {e + 1}: loss/pwc {loss_sum / max(n_steps, 1):.4f}  EPE/val {res['epe']:.4f}  "
                  f"Fl-all/val {res['fl_all']:.4f}  "
                  f"global_step {trainer.global_step}  {n_steps * args.batch_size * world / max(dt, 1e-9):.1f} pairs/s")
            os.makedirs(args.model_dir, exist_ok=True)
            ckpt.save_weights(os.path.join(args.model_dir, f"model_{e + 1}.ckpt"), trainer.state_dict())
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

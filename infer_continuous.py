#!/usr/bin/env python
"""Counterpart of the reference's test_continuous.py on the HIP path: flows between the
consecutive frames of an image sequence.

    python infer_continuous.py --input_images f0.png f1.png f2.png ... [--resume model_600.ckpt]

Follows reference test_continuous.py:45-64: frames are cropped to multiples of 64 and scaled to
[0,1]; every consecutive pair (i, i+1) goes through PWCDCNet; the 5-level flow pyramid is rescaled
to pixels per level (x 20 / 2^(6-l)).  Differences: consecutive pairs of equal size are run as ONE
batch (the reference feeds them one by one), and instead of a matplotlib figure each pair gets
<out>/<dname>/<fname>.png -- first frame and the colour-coded pyramid side by side -- plus
<out>/<dname>/<fname>.flo with the full-resolution flow.  --fit resize / pad keep the whole frame instead of cropping it: the
frames are uploaded as uint8, resized or padded to the next multiples of 64 on the GPU, and the .flo has the frame's own size
(the montage's pyramid levels stay at the network's geometry).
--chain K also writes, for every frame i whose K successors have its size, <out>/<dname>/<fname>_plus<K>.flo: the flow from frame i
to frame i + K, chained on the GPU from the K consecutive full-resolution flows (pwcnet_amd.chain_flows, across batch
boundaries; after the refit where --fit is not crop).  A pixel whose chain leaves the frame or meets an unknown flow holds the
.flo sentinel (flow_io.flow_valid).
--vis gpu builds every batch's montages in one launch on the GPU (pwcnet_amd.pyramid_montage): the pyramid levels are not copied
to the host, only the uint8 pictures and the full-resolution flow are; the .flo files do not depend on it.
--track SPEC also writes <out>/tracks.npy (frames, P, 2) float32 and <out>/tracks_status.npy (frames, P) uint8: where the query
points of SPEC are in every frame and what is known about them there (pwcnet_amd.track_points, across batch boundaries; after
the refit where --fit is not crop; positions (x, y) in the pixels of the frames the flow is computed on).  SPEC is grid:S, the
centres of S x S cells given in frame 0, or a text file of `frame x y` lines.  --track_fb also runs every batch's pairs reversed
and marks the points that fail the forward-backward check OCCLUDED.  The frames must all have one size.
--interp M also writes, for every consecutive pair, the M frames in between at t = k / (M + 1) as
<out>/<dname>/<fname>_t<k>of<M+1>.png (pwcnet_amd.interpolate_frames: both frames splatted along the two flows between them, one
call per batch; the reversed pairs are run as --track_fb runs them; after the refit where --fit is not crop).  Only the uint8
pictures come back to the host.  --interp_alpha A is the weight of the photometric match (exp(-A e)) [20].
--motion MODEL also writes <out>/motion.npy (pairs, 3, 3) float64 and <out>/motion_ok.npy (pairs,) bool: the dominant motion of
every pair, a translation, similarity or affine matrix taking a pixel (x, y, 1) of frame i to frame i + 1, fitted robustly on the
GPU (pwcnet_amd.fit_motion, one call per batch; after the refit where --fit is not crop; --motion homography: the eight-parameter
pwcnet_amd.fit_homography, and --motion_residual, --stabilize, --regions, --regions_track and --plate with --plate_foreground then
call their ops with projective=True, a division per pixel; --motion fundamental: pwcnet_amd.fit_fundamental, the epipolar
model for a camera that translates through depth -- motion.npy then holds the fundamental matrices, <out>/epipoles.npy (pairs, 3)
the homogeneous epipoles, --motion_residual writes <fname>_sampson.npy, every pixel's Sampson distance in pixels (1e10 where
unknown), in place of the residual .flo, --regions and --regions_track go through pwcnet_amd.epipolar_regions with
--regions_threshold as its threshold and the regions' mean flow itself in the table, and --stabilize and --plate, which need a
point map, are refused; --intrinsics FX FY CX CY, the camera's calibration in pixels, also writes <out>/pose.npy (pairs, 3, 4)
float64, [R | t] of pwcnet_amd.camera_pose with X' = R X + t and |t| = 1, all zeros where <out>/pose_ok.npy (pairs,) bool is False,
and with --depth, per pair, <fname>_depth.npy (float32, the depth in the first frame in baselines of THAT pair, 1e10 where unknown;
pwcnet_amd.triangulate_depth on the inliers of pwcnet_amd.epipolar_residual) and <fname>_depth.png, 8-bit inverse depth scaled to
the image's largest known inverse depth, 0 where unknown; --depth_min_parallax P switches pixels with less parallax off [0.25]); --pose_refine K (needs --intrinsics) refines every pose with K
passes of pwcnet_amd.refine_pose before anything uses it: pose.npy, the depth maps and the --trajectory chain are then the refined
poses', <out>/pose_closed.npy (pairs, 3, 4) keeps the closed form and <out>/pose_refine.npy (pairs, 4) float64 holds the rows
samples best_pass cost_first cost_best; a pair whose refinement is not ok keeps the closed form;
--trajectory (needs --intrinsics and frames of one size) chains the pairs' baselines on the GPU (pwcnet_amd.camera_trajectory,
across batch boundaries; the depth maps are computed for it whether or not --depth is given) and writes <out>/trajectory.npy
(frames, 3, 4) float64, world-to-camera [A | c] with X_cam = A X_world + c, the world being the first camera of the frame's segment,
<out>/scale.npy (pairs,) float64, <out>/segment.npy (pairs,) int32 and <out>/scale_links.npy (pairs, 2) float64 with the columns
ratio samples.  The --depth files stay in per-pair baselines: depth * scale[pair] is the depth in the unit of the pair's segment, the
baseline of that segment's first pair; a pair without a pose has scale 0 and segment -1, and a seam with fewer than
--trajectory_min_samples K samples [64] starts a new segment with a unit of its own.  Untuned, no loop closure: the scale drifts.
--motion_iters K and --motion_scale C
are the reweighting passes [4] and the Cauchy scale in pixels [1.0].  --motion_residual also writes <fname>_residual.flo, the flow
with that motion taken out (unknown pixels hold the .flo sentinel), and <fname>_inlier.png, white where a pixel moves with it.
--stabilize R (needs --motion and frames of one size) smooths the camera path over 2 R + 1 frames (pwcnet_amd.smooth_path) and, in
a second pass over the frames, writes <fname>_stab.png for every frame (pwcnet_amd.warp_frames).
--regions (needs --motion) also writes, per pair, <fname>_regions.png, a 16-bit greyscale PNG of the ids of the regions that move
on their own (pwcnet_amd.moving_regions: the connected components of the pixels whose flow is known and no inlier of the dominant
motion; ids in raster order of the regions' first pixels, saturating at 65535, 0 for the rest), and <fname>_regions.npy, a
(min(K, 256), 7) float64 table with the columns area x0 y0 x1 y1 mean_u mean_v (the box inclusive, the mean the region's motion
relative to the camera in pixels).  --regions_min_area A drops smaller regions [16], --regions_connectivity 4 or 8 [8],
--regions_threshold T is the inlier threshold in pixels [3.0].
--regions_track (needs --regions) also follows the regions from pair to pair (pwcnet_amd.track_regions, across batch boundaries): a
region of pair i is the region of pair i + 1 that most of its pixels land on under the flow i -> i + 1, where that one is also
fed mostly by it.  Per pair it writes <fname>_regions_ids.png, a 16-bit greyscale PNG of the regions' IDENTITIES (the same number for
the same object in every pair, saturating at 65535), and <fname>_regions_ids.npy, a (min(K, 256), 2) int32 table with the columns
identity age (row r: the region with id r + 1 in <fname>_regions.png; age: the consecutive pairs it has been seen in); at the end
<out>/regions_tracks.npy, int32 rows identity first_pair last_pair.  --regions_track_overlap K and --regions_track_fraction F: a link
needs at least K shared pixels [1] and at least F of the smaller region's area [0].  A change of the frame size starts new
identities.
--flow_filter R filters every pair's full-resolution flow before it is written or handed to any option above: the weighted median
over a (2 R + 1)^2 window, R = 1 .. 7, guided by the pair's first frame (pwcnet_amd.filter_flow; after the refit where --fit is not
crop, the reversed pairs' flows guided by their own first frame).  --flow_filter_sigma_space S (pixels) and
--flow_filter_sigma_color C (grey levels per channel) shape the weights [a box, no colour term], --flow_filter_iters K repeats it
[1].  The montage shows the network's pyramid and does not change.  Untuned: nobody has measured what it does to the error.
--denoise R also writes <out>/<dname>/<fname>_denoised.png for EVERY frame: the frame averaged with its R = 1 .. 8 neighbours on
either side along the flow (pwcnet_amd.temporal_filter, across batch boundaries; the reversed pairs are run as --track_fb runs
them; after the refit where --fit is not crop).  A neighbour weighs 1 / (1 + d^2 / S^2) by its patch's difference d in grey levels
(--denoise_sigma S [10], --denoise_patch P for (2 P + 1)^2 patches [1]) and is dropped where the forward-backward check fails
(--denoise_no_fb keeps it).  Only the uint8 pictures come back to the host.  The frames must all have one size.  Untuned: nobody
has measured the denoising quality on real footage.
--plate (needs --motion and frames of one size) writes, after the last pair, <out>/plate.png and <out>/plate_count.png: the
background plate of the sequence.  The dominant motions are chained from frame --plate_anchor A [0] (pwcnet_amd.plate_path; a pair
whose fit is degenerate cuts the chain, the frames beyond it are left out), the canvas is the box the reachable frames cover in the
anchor's coordinates grown by --plate_margin M [0] (pwcnet_amd.plate_canvas; an error where a side is above --plate_max_side S
[4096]), and at most --plate_frames K <= 64 [32] of the reachable frames, evenly spaced, are sampled at every canvas pixel on the GPU
(pwcnet_amd.background_plate): --plate_mode median [default] writes per channel the lower median of what the frames show there, so
that what moves on its own is voted out; mean averages.  plate_count.png holds the number of frames that see each pixel (the plate
is black where none does).  --plate_inliers lets a frame vote only where its pair's flow moves with the camera
(pwcnet_amd.motion_residual's inliers; the last frame votes everywhere).  --plate_foreground T also writes <fname>_fg.png for
every reachable frame, batch by batch (pwcnet_amd.plate_difference): white where the frame differs from the plate by more than T
grey levels in some channel, black where it does not, grey 128 where the plate is unknown.  Untuned: nobody has measured the
quality of the plate on real footage.
"""
import argparse
import os
import re
from glob import glob

import numpy as np
import torch


REGIONS_ROWS = 256                                   # --regions: the rows of a pair's table at most


def pyramid_montage(image, flows):
    """First frame followed by the colour-coded flows (coarse -> fine), all resized (nearest) to the
    frame's height, concatenated horizontally."""
    from pwcnet_amd import flow_io
    h = image.shape[0]
    tiles = [image]
    for f in flows:
        c = flow_io.flow_to_color(f)
        ry = np.arange(h) * c.shape[0] // h
        rx = np.arange(h * c.shape[1] // c.shape[0]) * c.shape[1] // (h * c.shape[1] // c.shape[0])
        tiles.append(c[ry][:, rx])
    return np.concatenate(tiles, axis=1)


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", "--input_images", type=str, nargs="+", required=True, help="Target images (required)")
    ap.add_argument("-r", "--resume", type=str, default=None, help="Learned parameter checkpoint prefix [None]")
    ap.add_argument("--out", type=str, default="./test_figure")
    ap.add_argument("--batch", type=int, default=8, help="pairs per forward")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--pipeline", type=int, default=3, help="forwards in flight (pwcnet_amd.ForwardPipeline depth; 1 = one at a time)")
    ap.add_argument("--fit", choices=("crop", "resize", "pad"), default="crop",
                    help="frames whose size is no multiple of 64: crop them (reference), or resize / pad them on the GPU and "
                         "bring the flow back to the frame's size [crop]")
    ap.add_argument("--normalize_features", action="store_true",
                    help="correlate layer-normalised feature maps (PWCDCNet(normalize_features=True)).  A checkpoint carries no marker for this: pass it exactly when the weights were trained with it")
    ap.add_argument("--norm_eps", type=float, default=1e-16, help="--normalize_features: epsilon under the square root [1e-16]")
    ap.add_argument("--chain", type=int, default=0, metavar="K",
                    help="also write <fname>_plus<K>.flo, the flow from frame i to frame i + K chained from the consecutive flows "
                         "on the GPU; unknown pixels hold the .flo sentinel [0: off]")
    ap.add_argument("--vis", choices=("host", "gpu"), default="host",
                    help="build the montages with numpy on the copied-back pyramid, or on the GPU (pwcnet_amd.pyramid_montage: only "
                         "uint8 pictures and the final flow cross to the host) [host]")
    ap.add_argument("--track", type=str, default=None, metavar="SPEC",
                    help="also write tracks.npy / tracks_status.npy: the query points of SPEC -- grid:S or a text file of "
                         "`frame x y` lines -- followed through the sequence on the GPU [off]")
    ap.add_argument("--track_fb", action="store_true",
                    help="--track: also run the reversed pairs and mark points that fail the forward-backward check OCCLUDED")
    ap.add_argument("--interp", type=_positive_int, default=0, metavar="M",
                    help="also write the M frames between every consecutive pair, <fname>_t<k>of<M+1>.png at t = k / (M + 1), "
                         "interpolated on the GPU from the two flows between them (the reversed pairs are run too) [off]")
    ap.add_argument("--interp_alpha", type=float, default=20.0, metavar="A",
                    help="--interp: the weight of a source pixel is exp(-min(A * e, 10)), e its match's mean colour error [20]")
    ap.add_argument("--motion", choices=("translation", "similarity", "affine", "homography", "fundamental"), default=None,
                    help="also write motion.npy / motion_ok.npy: the dominant motion of every pair, fitted robustly on the GPU; "
                         "homography: pwcnet_amd.fit_homography, and every flag below that uses the motion divides per pixel; "
                         "fundamental: pwcnet_amd.fit_fundamental, the epipolar model (also writes epipoles.npy; no --stabilize, no --plate) [off]")
    ap.add_argument("--intrinsics", type=float, nargs=4, default=None, metavar=("FX", "FY", "CX", "CY"),
                    help="--motion fundamental: the camera's focal lengths and principal point in pixels of the FRAMES (with --fit "
                         "resize the flow is refitted to the frames' own grid, so these need no scaling); also write pose.npy "
                         "(pairs, 3, 4), [R | t] with |t| = 1, and pose_ok.npy (pwcnet_amd.camera_pose) [off]")
    ap.add_argument("--pose_refine", type=int, default=0, metavar="K",
                    help="--intrinsics: refine every pose with K passes of pwcnet_amd.refine_pose (the --motion_scale weight, the 1 px "
                         "inlier gate); pose.npy, the --depth files and the --trajectory chain then use the refined poses, "
                         "pose_closed.npy (pairs, 3, 4) keeps camera_pose's and pose_refine.npy (pairs, 4) holds the rows samples "
                         "best_pass cost_first cost_best [0: off]")
    ap.add_argument("--depth", action="store_true",
                    help="--intrinsics: also write <fname>_depth.npy (float32 depth in baselines of that pair, 1e10 where unknown) "
                         "and <fname>_depth.png (8-bit inverse depth, 0 where unknown) for every pair")
    ap.add_argument("--depth_min_parallax", type=float, default=0.25, metavar="P",
                    help="--depth: pixels with less than P pixels of parallax are unknown [0.25]")
    ap.add_argument("--trajectory", action="store_true",
                    help="--intrinsics: also write trajectory.npy (frames, 3, 4), scale.npy, segment.npy and scale_links.npy: the "
                         "pairs' baselines chained into one unit per segment and the camera's path, on the GPU")
    ap.add_argument("--trajectory_min_samples", type=_positive_int, default=64, metavar="K",
                    help="--trajectory: a seam links two pairs' scales only with at least K samples [64]")
    ap.add_argument("--motion_iters", type=int, default=4, metavar="K", help="--motion: reweighting passes, 0 .. 64 [4]")
    ap.add_argument("--motion_scale", type=float, default=1.0, metavar="C", help="--motion: the Cauchy scale in pixels [1.0]")
    ap.add_argument("--motion_residual", action="store_true",
                    help="--motion: also write <fname>_residual.flo and <fname>_inlier.png for every pair")
    ap.add_argument("--stabilize", type=int, default=0, metavar="R",
                    help="--motion: also write <fname>_stab.png for every frame, the camera path smoothed over 2 R + 1 frames [0: off]")
    ap.add_argument("--regions", action="store_true",
                    help="--motion: also write <fname>_regions.png (16-bit ids) and <fname>_regions.npy (area x0 y0 x1 y1 mean_u "
                         "mean_v) for every pair: the regions that move on their own, labelled on the GPU")
    ap.add_argument("--regions_min_area", type=_positive_int, default=16, metavar="A", help="--regions: drop regions below A pixels [16]")
    ap.add_argument("--regions_connectivity", type=int, choices=(4, 8), default=8, help="--regions: shared edges, or edges and corners [8]")
    ap.add_argument("--regions_threshold", type=float, default=3.0, metavar="T",
                    help="--regions: a pixel moves with the camera where its residual is at most T pixels [3.0]")
    ap.add_argument("--regions_track", action="store_true",
                    help="--regions: also write <fname>_regions_ids.png / .npy for every pair and regions_tracks.npy: the regions "
                         "followed from pair to pair on the GPU, one identity per object")
    ap.add_argument("--regions_track_overlap", type=_positive_int, default=1, metavar="K",
                    help="--regions_track: a link needs at least K shared pixels [1]")
    ap.add_argument("--regions_track_fraction", type=float, default=0.0, metavar="F",
                    help="--regions_track: a link needs at least F of the smaller region's area, 0 .. 1 [0]")
    from pwcnet_amd.flow_filter import add_cli_arguments
    add_cli_arguments(ap)
    from pwcnet_amd.temporal import add_cli_arguments as add_denoise_arguments
    add_denoise_arguments(ap)
    from pwcnet_amd.plate import add_cli_arguments as add_plate_arguments
    add_plate_arguments(ap)
    return ap


def _positive_int(text):
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError(f"expected an integer >= 1, got {text!r}")
    return value


def parse_track_spec(spec, nframes, H, W):
    """(points (P,2) float32 (x, y), start (P,) int32) of --track SPEC for a sequence of nframes H x W frames: `grid:S`, the
    centres of S x S cells (pwcnet_amd.grid_points) given in frame 0, or the path of a text file with one `frame x y` per line
    (blank lines and #-comments are skipped)."""
    if spec.startswith("grid:"):
        try:
            stride = int(spec[5:])
        except ValueError:
            stride = 0
        if stride < 1:
            raise ValueError(f"--track: expected grid:S with a positive integer S, got {spec!r}")
        from pwcnet_amd.track import grid_points
        points = grid_points(H, W, stride).numpy()
        return points, np.zeros(points.shape[0], np.int32)
    if not os.path.isfile(spec):
        raise ValueError(f"--track: expected grid:S or the path of a text file of `frame x y` lines, got {spec!r}")
    points, start = [], []
    with open(spec) as f:
        for no, line in enumerate(f, 1):
            fields = line.split("#", 1)[0].split()
            if not fields:
                continue
            try:
                frame, x, y = int(fields[0]), float(fields[1]), float(fields[2])
                if len(fields) != 3:
                    raise ValueError
            except (ValueError, IndexError):
                raise ValueError(f"--track: {spec}:{no}: expected `frame x y`, got {line.strip()!r}") from None
            if not 0 <= frame < nframes:
                raise ValueError(f"--track: {spec}:{no}: frame {frame} is outside the sequence of {nframes} frames")
            points.append((x, y))
            start.append(frame)
    if not points:
        raise ValueError(f"--track: {spec} holds no query point")
    return np.asarray(points, np.float32).reshape(-1, 2), np.asarray(start, np.int32)


def out_stem(path):
    """(dname, fname) of a frame's outputs under --out."""
    parts = re.split("[/.]", path)
    return parts[-3:-1] if len(parts) >= 3 else ("", parts[-2])


def inverse_depth_picture(depth):
    """--depth: the (H, W) uint8 picture of a downloaded depth map -- inverse depth over the image's largest known inverse depth,
    times 255 and rounded; 0 where the depth is unknown (the 1e10 sentinel)."""
    known = np.abs(depth) <= np.float32(1e9)
    inverse = np.where(known, 1.0 / np.where(known, depth, np.float32(1.0)).astype(np.float64), 0.0)
    top = inverse.max() if known.any() else 0.0
    return np.rint(inverse * (255.0 / top)).astype(np.uint8) if top > 0.0 else np.zeros(depth.shape, np.uint8)


class Chainer:
    """--chain K: takes the full-resolution flows i -> i + 1 as they come, batch after batch, keeps the last ones on the GPU and
    writes <fname>_plus<K>.flo for every frame i whose K successors have its size as soon as its K flows are there."""

    def __init__(self, span, frames, paths, out):
        self.span, self.frames, self.paths, self.out = span, frames, paths, out
        self.held = {}                               # pair index i -> its (H,W,2) flow on the GPU
        self.next = 0                                # the first frame whose chain is not written yet

    def add(self, first, flows):
        """flows: (n,H,W,2) on the GPU, the flows of the pairs first, first + 1, ..."""
        import pwcnet_amd
        from pwcnet_amd import flow_io
        K = self.span
        for k in range(flows.shape[0]):
            self.held[first + k] = flows[k]
        last = first + flows.shape[0] - 1            # every pair up to here is held or done
        while self.next + K - 1 <= last:
            i0 = self.next
            if any(self.frames[i0 + d].shape != self.frames[i0].shape for d in range(1, K + 1)):
                self.next += 1
                continue
            i1 = i0                                  # frames i0 .. i1 start a chain over frames of one size
            while i1 + K <= last and self.frames[i1 + K + 1].shape == self.frames[i0].shape:
                i1 += 1
            seq = torch.stack([self.held[i] for i in range(i0, i1 + K)])
            chained = pwcnet_amd.chain_flows(seq, span=K)[0].cpu().numpy()
            for i in range(i0, i1 + 1):
                dname, fname = out_stem(self.paths[i])
                os.makedirs(os.path.join(self.out, dname), exist_ok=True)
                flow_io.write_flo(os.path.join(self.out, dname, f"{fname}_plus{K}.flo"), chained[i - i0])
            self.next = i1 + 1
        for i in [i for i in self.held if i < self.next]:
            del self.held[i]


class Tracker:
    """--track: takes the full-resolution flows i -> i + 1 (and, --track_fb, i + 1 -> i) as they come, batch after batch, steps
    the query points through them (pwcnet_amd.track_points) and keeps only the (P,2) positions and (P,) states of the last frame
    seen on the GPU; save() writes the (frames, P, 2) tracks and (frames, P) states."""

    def __init__(self, points, start, nframes, out):
        self.start = torch.from_numpy(np.asarray(start, np.int32)).cuda()
        self.points = torch.from_numpy(np.asarray(points, np.float32)).cuda()
        self.state = torch.zeros(self.points.shape[0], dtype=torch.uint8, device="cuda")       # UNSEEN: not started yet
        self.tracks = np.zeros((nframes, self.points.shape[0], 2), np.float32)
        self.status = np.zeros((nframes, self.points.shape[0]), np.uint8)
        self.out = out

    def add(self, first, flows_fw, flows_bw=None):
        """flows_fw: (n,H,W,2) on the GPU, the flows of the pairs first, first + 1, ...; flows_bw: the flows of the reversed
        pairs.  A point not started yet starts at start - first (beyond this batch: not in this call)."""
        import pwcnet_amd
        n = flows_fw.shape[0]
        tracks, status = pwcnet_amd.track_points(flows_fw, self.points, flows_bw=flows_bw, start=(self.start - first).clamp_(min=0),
                                                 status=self.state)
        self.points, self.state = tracks[n], status[n]
        self.tracks[first:first + n + 1] = tracks.cpu().numpy()
        self.status[first:first + n + 1] = status.cpu().numpy()

    def save(self):
        os.makedirs(self.out, exist_ok=True)
        np.save(os.path.join(self.out, "tracks.npy"), self.tracks)
        np.save(os.path.join(self.out, "tracks_status.npy"), self.status)


class Denoiser:
    """--denoise R: takes the uint8 frames at the flows' size and the full-resolution flows i -> i + 1 and i + 1 -> i as they come,
    batch after batch, keeps the frames and flows the pieces still to come need on the GPU (the last 2 R frames once a piece is
    done) and writes <fname>_denoised.png for the frames of every piece of pwcnet_amd.plan_windows as soon as its clip is there --
    the last R frames of the sequence with the last batch."""

    def __init__(self, kwargs, nframes, batch, paths, out):
        import pwcnet_amd
        self.kwargs, self.paths, self.out = kwargs, paths, out
        self.pieces = pwcnet_amd.plan_windows(nframes, kwargs["radius"], max(1, batch))
        self.frames, self.fw, self.bw = {}, {}, {}   # frame / pair index -> its tensor on the GPU

    def add(self, first, pictures, flows_fw, flows_bw):
        """pictures: (n + 1,H,W,3) uint8 on the GPU, the frames first, first + 1, ...; flows_fw, flows_bw: (n,H,W,2), the flows
        of the pairs first, first + 1, ... and of the reversed pairs."""
        import pwcnet_amd
        from PIL import Image
        n = flows_fw.shape[0]
        for k in range(n + 1):
            self.frames[first + k] = pictures[k]
        for k in range(n):                           # (the replica writes its result buffers again at its next forward)
            self.fw[first + k], self.bw[first + k] = flows_fw[k].clone(), flows_bw[k].clone()
        while self.pieces and self.pieces[0][1] - 1 <= first + n:
            cs, ce, o0, o1 = self.pieces.pop(0)
            clip = torch.stack([self.frames[i] for i in range(cs, ce)])
            fw = torch.stack([self.fw[i] for i in range(cs, ce - 1)]) if ce - cs > 1 else None
            bw = torch.stack([self.bw[i] for i in range(cs, ce - 1)]) if ce - cs > 1 else None
            denoised = pwcnet_amd.temporal_filter(clip, fw, bw, out_range=(o0 - cs, o1 - cs), **self.kwargs)[0].cpu().numpy()
            for i in range(o0, o1):
                dname, fname = out_stem(self.paths[i])
                os.makedirs(os.path.join(self.out, dname), exist_ok=True)
                Image.fromarray(denoised[i - o0]).save(os.path.join(self.out, dname, fname + "_denoised.png"))
            keep = self.pieces[0][0] if self.pieces else first + n + 1
            for held in (self.frames, self.fw, self.bw):
                for i in [i for i in held if i < keep]:
                    del held[i]


class PathChainer:
    """--trajectory: takes the full-resolution flows, poses, depth maps and known masks of the pairs as they come, batch after
    batch, chains their baselines (pwcnet_amd.camera_trajectory; the last pair stays on the GPU as the state) and keeps the rows on
    the host; save() writes the four files."""

    def __init__(self, nframes, intrinsics, min_samples, out):
        self.intrinsics, self.min_samples, self.out = intrinsics, min_samples, out
        self.state = None
        self.trajectory = np.zeros((nframes, 3, 4), np.float64)
        self.scale = np.zeros(nframes - 1, np.float64)
        self.segment = np.zeros(nframes - 1, np.int32)
        self.links = np.zeros((nframes - 1, 2), np.float64)

    def add(self, first, flows, rotation, translation, depth, known):
        import pwcnet_amd
        n = flows.shape[0]
        trajectory, scales, segment, info, state = pwcnet_amd.camera_trajectory(
            flows, rotation, translation, self.intrinsics, depth, known, min_samples=self.min_samples, state=self.state)
        state["flow"] = state["flow"].clone()        # (the replica writes its result buffer again at its next forward)
        self.state = state
        self.trajectory[first:first + n + 1] = trajectory.cpu().numpy()       # row 0 replaces the last row of the batch before
        self.scale[first:first + n], self.segment[first:first + n] = scales.cpu().numpy(), segment.cpu().numpy()
        self.links[first:first + n, 0], self.links[first:first + n, 1] = info["ratio"].cpu().numpy(), info["samples"].cpu().numpy()

    def save(self):
        os.makedirs(self.out, exist_ok=True)
        np.save(os.path.join(self.out, "trajectory.npy"), self.trajectory)
        np.save(os.path.join(self.out, "scale.npy"), self.scale)
        np.save(os.path.join(self.out, "segment.npy"), self.segment)
        np.save(os.path.join(self.out, "scale_links.npy"), self.links)


class RegionTracker:
    """--regions_track: takes the labels, counts, tables and full-resolution flows of the pairs as they come, batch after batch,
    gives every region its identity (pwcnet_amd.track_regions; the last pair's labels, table, ids and flow stay on the GPU as
    the state) and writes the two files of every pair; save() writes the identities' first and last pairs."""

    def __init__(self, paths, out, min_overlap, min_fraction):
        self.paths, self.out, self.min_overlap, self.min_fraction = paths, out, min_overlap, min_fraction
        self.state = None
        self.spans = {}                              # identity -> [first pair, last pair]

    def add(self, first, labels, count, regions, flows):
        """labels, count, regions: moving_regions' of the pairs first, first + 1, ...; flows: (n,H,W,2) on the GPU, theirs."""
        import pwcnet_amd
        from PIL import Image
        if self.state is not None and tuple(self.state["labels"].shape) != tuple(labels.shape[1:]):
            self.state = {"ids": torch.zeros_like(self.state["ids"]), "age": torch.zeros_like(self.state["age"]),
                          "next_id": self.state["next_id"], "next_id_bound": self.state["next_id_bound"],
                          "labels": torch.zeros_like(labels[0]), "area": self.state["area"], "count": self.state["count"],
                          "flow": torch.zeros_like(flows[0]), "valid": None}       # another frame size: nothing links, ids go on
        ids, age, _, self.state = pwcnet_amd.track_regions(labels, count, regions, flows, state=self.state,
                                                           min_overlap=self.min_overlap, min_fraction=self.min_fraction)
        painted = pwcnet_amd.relabel_regions(labels, ids).clamp(max=65535).cpu().numpy().astype(np.uint16)
        table, count = torch.stack([ids, age], dim=2).cpu().numpy(), count.cpu().numpy()
        for k in range(labels.shape[0]):
            dname, fname = out_stem(self.paths[first + k])
            os.makedirs(os.path.join(self.out, dname), exist_ok=True)
            rows = table[k, :min(int(count[k]), REGIONS_ROWS)]
            Image.fromarray(painted[k]).save(os.path.join(self.out, dname, fname + "_regions_ids.png"))
            np.save(os.path.join(self.out, dname, fname + "_regions_ids.npy"), rows)
            for identity in rows[:, 0].tolist():
                self.spans.setdefault(identity, [first + k, first + k])[1] = first + k

    def save(self):
        os.makedirs(self.out, exist_ok=True)
        rows = [[identity, span[0], span[1]] for identity, span in sorted(self.spans.items())]
        np.save(os.path.join(self.out, "regions_tracks.npy"), np.asarray(rows, np.int32).reshape(-1, 3))


def main():
    ap = build_parser()
    args = ap.parse_args()
    paths = []
    for p in args.input_images:                      # expand wild-cards (test_continuous.py:75-78)
        paths.extend(sorted(glob(p)) if "*" in p else [p])
    if len(paths) < 2:
        raise ValueError("# of input images must be >= 2")
    if args.chain < 0 or args.chain >= len(paths):
        ap.error(f"--chain must be at least 0 and below the number of frames ({len(paths)}), got {args.chain}")

    if args.track_fb and args.track is None:
        ap.error("--track_fb needs --track SPEC")
    if args.interp > 16:
        ap.error(f"--interp must be at most 16 (pwcnet_amd.interp.MAX_TIMES), got {args.interp}")
    if not args.interp_alpha >= 0.0:
        ap.error(f"--interp_alpha must be non-negative, got {args.interp_alpha}")
    from pwcnet_amd.temporal import check_cli_arguments as check_denoise_arguments
    denoise = check_denoise_arguments(ap, args)      # temporal_filter's keyword arguments, None without --denoise
    # the reversed pairs are run too: one ticket serves the three flags
    both_ways = args.track_fb or args.interp > 0 or denoise is not None
    if args.motion is None and (args.motion_residual or args.stabilize != 0):
        ap.error("--motion_residual and --stabilize need --motion MODEL")
    if args.motion == "fundamental" and (args.stabilize != 0 or args.plate):
        ap.error("--stabilize and --plate need a point map; --motion fundamental is a constraint, not one: use affine or homography")
    if args.intrinsics is not None and args.motion != "fundamental":
        ap.error("--intrinsics needs --motion fundamental: the pose comes from the fundamental matrix")
    if args.depth and args.intrinsics is None:
        ap.error("--depth needs --intrinsics FX FY CX CY")
    if args.pose_refine and args.intrinsics is None:
        ap.error("--pose_refine needs --intrinsics FX FY CX CY")
    if not 0 <= args.pose_refine <= 64:
        ap.error(f"--pose_refine must be in 0 .. 64, got {args.pose_refine}")
    if args.trajectory and (args.motion != "fundamental" or args.intrinsics is None):
        ap.error("--trajectory needs --motion fundamental --intrinsics FX FY CX CY")
    if not args.depth_min_parallax >= 0.0:
        ap.error(f"--depth_min_parallax must be non-negative, got {args.depth_min_parallax}")
    if args.regions and args.motion is None:
        ap.error("--regions needs --motion MODEL")
    if args.regions_track and not args.regions:
        ap.error("--regions_track needs --regions")
    if not 0.0 <= args.regions_track_fraction <= 1.0:
        ap.error(f"--regions_track_fraction must be in 0 .. 1, got {args.regions_track_fraction}")
    if not args.regions_threshold >= 0.0:
        ap.error(f"--regions_threshold must be non-negative, got {args.regions_threshold}")
    if not 0 <= args.motion_iters <= 64:
        ap.error(f"--motion_iters must be in 0 .. 64, got {args.motion_iters}")
    if not args.motion_scale > 0.0:
        ap.error(f"--motion_scale must be positive, got {args.motion_scale}")
    if args.stabilize < 0:
        ap.error(f"--stabilize must be at least 0, got {args.stabilize}")
    from pwcnet_amd.plate import check_cli_arguments as check_plate_arguments
    plate_on = check_plate_arguments(ap, args, len(paths))
    from pwcnet_amd.flow_filter import check_cli_arguments
    filt = check_cli_arguments(ap, args)             # filter_flow's keyword arguments, None without --flow_filter

    from PIL import Image
    import pwcnet_amd
    from pwcnet_amd import ckpt, flow_io

    torch.cuda.set_device(args.gpu)
    # Round 6: the batches of a sequence are independent forwards -- dealt to the replicas of a ForwardPipeline (HIP streams with
    # hardware queues of their own) the launch-bound coarse levels of one batch run under the matrix-bound launches of another.
    # Results are read behind pipeline.synchronize(): every forward has then passed its fp16-range check (a flagged one has been
    # repeated on the fp32 kernels), which is what range_check="sync" gave the one-forward-at-a-time loop.
    model = pwcnet_amd.ForwardPipeline(depth=args.pipeline, normalize_features=args.normalize_features, norm_eps=args.norm_eps)
    if args.resume is not None:
        print(f"Loading learned model from checkpoint {args.resume}")
        model.load_weights(ckpt.load_weights(args.resume))
    else:
        print("!!! Test with un-learned model !!!")

    frames = [np.asarray(Image.open(p).convert("RGB")) for p in paths]
    if args.fit == "crop":
        frames = [flow_io.factor_crop(f) for f in frames]
    # runs of consecutive pairs whose frames all have one size: one batch each
    jobs = []
    i = 0
    while i < len(frames) - 1:
        j = i
        while j < len(frames) - 1 and j - i < args.batch and frames[j + 1].shape == frames[i].shape:
            j += 1
        if j == i:
            raise ValueError(f"{paths[i]} and {paths[i + 1]} differ in size" + (" after cropping" if args.fit == "crop" else ""))
        jobs.append((i, j))
        i = j
    num_levels = model.nets[0].num_levels
    chainer = Chainer(args.chain, frames, paths, args.out) if args.chain > 0 else None
    tracker = None
    if args.track is not None:
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError("--track needs frames of one size" + (" after cropping" if args.fit == "crop" else ""))
        tracker = Tracker(*parse_track_spec(args.track, len(frames), *frames[0].shape[:2]), len(frames), args.out)
    denoiser = None
    if denoise is not None:
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError("--denoise needs frames of one size" + (" after cropping" if args.fit == "crop" else ""))
        denoiser = Denoiser(denoise, len(frames), args.batch, paths, args.out)
    region_tracker = None
    if args.regions_track:
        region_tracker = RegionTracker(paths, args.out, args.regions_track_overlap, args.regions_track_fraction)
    path_chainer = None
    if args.trajectory:
        if any(f.shape != frames[0].shape for f in frames):
            raise ValueError("--trajectory needs frames of one size" + (" after cropping" if args.fit == "crop" else ""))
        path_chainer = PathChainer(len(frames), args.intrinsics, args.trajectory_min_samples, args.out)
    motions, motions_ok = [None] * (len(frames) - 1), [None] * (len(frames) - 1)
    epipolar = args.motion == "fundamental"
    epipoles = [None] * (len(frames) - 1) if epipolar else None
    poses, poses_ok = ([None] * (len(frames) - 1), [None] * (len(frames) - 1)) if args.intrinsics is not None else (None, None)
    poses_closed, poses_refine = [None] * (len(frames) - 1), [None] * (len(frames) - 1)      # --pose_refine
    proj = {"projective": True} if args.motion == "homography" else {}       # the other models: the calls as they were
    if args.stabilize > 0 and any(f.shape != frames[0].shape for f in frames):
        raise ValueError("--stabilize needs frames of one size" + (" after cropping" if args.fit == "crop" else ""))
    if plate_on and any(f.shape != frames[0].shape for f in frames):
        raise ValueError("--plate needs frames of one size" + (" after cropping" if args.fit == "crop" else ""))
    plate_inliers = [None] * len(frames) if plate_on and args.plate_inliers else None
    window = 2 * max(1, args.pipeline)               # batches submitted before the first one is read back
    if both_ways:
        window = max(1, args.pipeline)               # (two forwards per batch)
    for w0 in range(0, len(jobs), window):
        tickets = []
        for i, j in jobs[w0:w0 + window]:
            pictures = None                          # --interp, --denoise: the uint8 frames at the flows' size
            if args.fit == "crop":
                seq = torch.from_numpy(np.stack(frames[i:j + 1]).astype(np.float32) / 255.0).cuda()
                info, shown = None, seq              # (a float32 frame made as u8 / 255 gives back u8)
                if args.interp > 0 or denoiser is not None:
                    pictures = torch.from_numpy(np.stack(frames[i:j + 1])).cuda()
            else:                                    # uint8 upload; / 255 and the fit in one launch on the caller's stream
                shown = torch.from_numpy(np.stack(frames[i:j + 1])).cuda()
                seq, info = pwcnet_amd.fit_frames(shown, args.fit)
                pictures = shown
            first, second = seq[:-1].contiguous(), seq[1:].contiguous()
            tickets.append((i, j, info, shown if args.vis == "gpu" else None, model.submit(first, second),
                            model.submit(second, first) if both_ways else None,
                            pictures if args.interp > 0 or denoiser is not None else None))
        model.synchronize()
        for i, j, info, shown, ticket, reverse, pictures in tickets:
            flow_final, flows = ticket.result()
            if info is not None:
                flow_final = pwcnet_amd.refit_flow(flow_final, info)
            flow_back = None
            if reverse is not None:
                flow_back = reverse.result()[0]
                if info is not None:
                    flow_back = pwcnet_amd.refit_flow(flow_back, info)
            if filt is not None:                     # the frames at the flow's geometry are the guides; uint8 upload
                guides = torch.from_numpy(np.stack(frames[i:j + 1])).cuda()
                flow_final = pwcnet_amd.filter_flow(flow_final, guide=guides[:-1], **filt)[0]
                if flow_back is not None:
                    flow_back = pwcnet_amd.filter_flow(flow_back, guide=guides[1:], **filt)[0]
            if chainer is not None:
                chainer.add(i, flow_final.clone())   # (the replica writes its result buffer again at its next forward)
            if tracker is not None:
                tracker.add(i, flow_final, flow_back if args.track_fb else None)
            if args.interp > 0:                      # one call per batch; only the uint8 pictures cross to the host
                between = pwcnet_amd.interpolate_frames(pictures[:-1], pictures[1:], flow_final, flow_back,
                                                        [k / (args.interp + 1) for k in range(1, args.interp + 1)],
                                                        alpha=args.interp_alpha)[0].cpu().numpy()
                for k in range(j - i):
                    dname, fname = out_stem(paths[i + k])
                    os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                    for m in range(args.interp):
                        Image.fromarray(between[k, m]).save(os.path.join(args.out, dname, f"{fname}_t{m + 1}of{args.interp + 1}.png"))
            if denoiser is not None:                 # only the uint8 pictures cross to the host
                denoiser.add(i, pictures, flow_final, flow_back)
            if args.motion is not None:              # one call per batch; matrices, flags and uint8 pictures cross to the host
                if epipolar:
                    matrices, ok, fit_info = pwcnet_amd.fit_fundamental(flow_final, iters=args.motion_iters, scale=args.motion_scale)
                    epipoles[i:j] = list(fit_info["epipole"].cpu().numpy())
                    if poses is not None:            # the pose, flags and (--depth) the depth maps cross to the host
                        rotation, translation, pose_ok, _ = pwcnet_amd.camera_pose(flow_final, matrices, args.intrinsics)
                        if args.pose_refine:         # the closed form is kept beside the refined pose
                            poses_closed[i:j] = list(torch.cat([rotation, translation[:, :, None]], dim=2).cpu().numpy())
                            refined, moved, refine_ok, refine_info = pwcnet_amd.refine_pose(
                                flow_final, rotation, translation, args.intrinsics, iters=args.pose_refine, scale=args.motion_scale)
                            rotation = torch.where(refine_ok[:, None, None], refined, rotation)
                            translation = torch.where(refine_ok[:, None], moved, translation)
                            cost = refine_info["cost"]
                            cost_best = cost.gather(1, refine_info["best_pass"].long()[:, None])[:, 0]
                            poses_refine[i:j] = list(torch.stack([refine_info["samples"].double(), refine_info["best_pass"].double(),
                                                                  cost[:, 0], cost_best], dim=1).cpu().numpy())
                        poses[i:j] = list(torch.cat([rotation, translation[:, :, None]], dim=2).cpu().numpy())
                        poses_ok[i:j] = list(pose_ok.cpu().numpy())
                        if args.depth or path_chainer is not None:
                            inlier = pwcnet_amd.epipolar_residual(flow_final, matrices)[1]
                            depth, depth_known = pwcnet_amd.triangulate_depth(flow_final, rotation, translation, args.intrinsics,
                                                                              valid=inlier, min_parallax=args.depth_min_parallax)
                            if path_chainer is not None:     # the maps stay on the GPU for it; four small arrays cross to the host
                                path_chainer.add(i, flow_final, rotation, translation, depth, depth_known)
                            depth = depth.cpu().numpy() if args.depth else None
                            for k in range(j - i if args.depth else 0):
                                dname, fname = out_stem(paths[i + k])
                                os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                                np.save(os.path.join(args.out, dname, fname + "_depth.npy"), depth[k])
                                Image.fromarray(inverse_depth_picture(depth[k])).save(os.path.join(args.out, dname, fname + "_depth.png"))
                elif args.motion == "homography":
                    matrices, ok, _ = pwcnet_amd.fit_homography(flow_final, iters=args.motion_iters, scale=args.motion_scale)
                else:
                    matrices, ok, _ = pwcnet_amd.fit_motion(flow_final, model=args.motion, iters=args.motion_iters,
                                                            scale=args.motion_scale)
                motions[i:j], motions_ok[i:j] = list(matrices.cpu().numpy()), list(ok.cpu().numpy())
                if plate_inliers is not None:        # --plate_inliers: the masks wait on the host for the second pass
                    plate_inliers[i:j] = list(pwcnet_amd.motion_residual(flow_final, matrices, **proj)[1].to(torch.uint8).cpu().numpy())
                if args.motion_residual and epipolar:
                    distance, inlier = pwcnet_amd.epipolar_residual(flow_final, matrices)
                    distance, inlier = distance.cpu().numpy(), (inlier.to(torch.uint8) * 255).cpu().numpy()
                    for k in range(j - i):
                        dname, fname = out_stem(paths[i + k])
                        os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                        np.save(os.path.join(args.out, dname, fname + "_sampson.npy"), distance[k])
                        Image.fromarray(inlier[k]).save(os.path.join(args.out, dname, fname + "_inlier.png"))
                elif args.motion_residual:
                    residual, inlier = pwcnet_amd.motion_residual(flow_final, matrices, **proj)
                    residual, inlier = residual.cpu().numpy(), (inlier.to(torch.uint8) * 255).cpu().numpy()
                    for k in range(j - i):
                        dname, fname = out_stem(paths[i + k])
                        os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                        flow_io.write_flo(os.path.join(args.out, dname, fname + "_residual.flo"), residual[k])
                        Image.fromarray(inlier[k]).save(os.path.join(args.out, dname, fname + "_inlier.png"))
                if args.regions:                     # the ids and the tables cross to the host, nothing else
                    find_regions = pwcnet_amd.epipolar_regions if epipolar else pwcnet_amd.moving_regions
                    labels, count, regions = find_regions(
                        flow_final, matrices, threshold=args.regions_threshold, connectivity=args.regions_connectivity,
                        min_area=args.regions_min_area, max_regions=REGIONS_ROWS, **proj)[:3]
                    if region_tracker is not None:   # (before the host copies below take the names)
                        region_tracker.add(i, labels, count, regions, flow_final)
                    labels, count = labels.clamp(max=65535).cpu().numpy().astype(np.uint16), count.cpu().numpy()
                    table = np.concatenate([regions["area"].cpu().numpy()[..., None].astype(np.float64),
                                            regions["box"].cpu().numpy().astype(np.float64), regions["mean"].cpu().numpy()], axis=2)
                    for k in range(j - i):
                        dname, fname = out_stem(paths[i + k])
                        os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                        Image.fromarray(labels[k]).save(os.path.join(args.out, dname, fname + "_regions.png"))
                        np.save(os.path.join(args.out, dname, fname + "_regions.npy"), table[k, :min(int(count[k]), REGIONS_ROWS)])
            flow_final = flow_final.cpu().numpy()
            scales = [20.0 / 2 ** (num_levels - l) for l in range(len(flows))]
            if args.vis == "gpu":                    # one launch per batch; the pyramid stays on the GPU
                montages = pwcnet_amd.pyramid_montage(shown[:-1], list(flows), scales).cpu().numpy()
            else:
                flows = [f.cpu().numpy() for f in flows]
            for k in range(j - i):
                dname, fname = out_stem(paths[i + k])
                os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                if args.vis == "gpu":
                    montage = montages[k]
                else:
                    montage = pyramid_montage(frames[i + k], [f[k] * s for f, s in zip(flows, scales)])
                Image.fromarray(montage).save(os.path.join(args.out, dname, fname + ".png"))
                flow_io.write_flo(os.path.join(args.out, dname, fname + ".flo"), flow_final[k])
    if tracker is not None:
        tracker.save()
    if region_tracker is not None:
        region_tracker.save()
    if path_chainer is not None:
        path_chainer.save()
    if args.motion is not None:
        os.makedirs(args.out, exist_ok=True)
        np.save(os.path.join(args.out, "motion.npy"), np.stack(motions))
        np.save(os.path.join(args.out, "motion_ok.npy"), np.asarray(motions_ok, bool))
        if epipolar:
            np.save(os.path.join(args.out, "epipoles.npy"), np.stack(epipoles))
        if poses is not None:
            np.save(os.path.join(args.out, "pose.npy"), np.stack(poses))
            if args.pose_refine:
                np.save(os.path.join(args.out, "pose_closed.npy"), np.stack(poses_closed))
                np.save(os.path.join(args.out, "pose_refine.npy"), np.stack(poses_refine))
            np.save(os.path.join(args.out, "pose_ok.npy"), np.asarray(poses_ok, bool))
    if args.stabilize > 0:                           # the second pass: the frames again, batch by batch
        steady = pwcnet_amd.smooth_path(np.stack(motions), args.stabilize, **proj)
        for i in range(0, len(frames), max(1, args.batch)):
            j = min(i + max(1, args.batch), len(frames))
            stab = pwcnet_amd.warp_frames(torch.from_numpy(np.stack(frames[i:j])).cuda(), steady[i:j], **proj)[0].cpu().numpy()
            for k in range(j - i):
                dname, fname = out_stem(paths[i + k])
                os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                Image.fromarray(stab[k]).save(os.path.join(args.out, dname, fname + "_stab.png"))
    if plate_on:                                     # the second pass: the chosen frames in one call, then every frame against it
        from pwcnet_amd.plate import select_frames
        H, W = frames[0].shape[:2]
        to_frame, reach = pwcnet_amd.plate_path(np.stack(motions), np.asarray(motions_ok, bool), anchor=args.plate_anchor, **proj)
        x0, y0, Hc, Wc = pwcnet_amd.plate_canvas(to_frame, reach, H, W, margin=args.plate_margin, max_side=args.plate_max_side, **proj)
        to_canvas_frame, to_canvas = pwcnet_amd.canvas_matrices(to_frame, x0, y0, **proj)
        chosen = select_frames(reach, args.plate_anchor, args.plate_frames)
        masks = None
        if plate_inliers is not None:
            masks = torch.from_numpy(np.stack([np.ones((H, W), np.uint8) if plate_inliers[i] is None else plate_inliers[i]
                                               for i in chosen])).cuda()
        plate, count = pwcnet_amd.background_plate(torch.from_numpy(np.stack([frames[i] for i in chosen])).cuda(),
                                                   to_canvas_frame[chosen], (Hc, Wc), mode=args.plate_mode, masks=masks, **proj)
        os.makedirs(args.out, exist_ok=True)
        Image.fromarray(plate.cpu().numpy()).save(os.path.join(args.out, "plate.png"))
        Image.fromarray(count.cpu().numpy()).save(os.path.join(args.out, "plate_count.png"))
        if args.plate_foreground is not None:
            reachable = [int(i) for i in np.nonzero(reach)[0]]
            for b in range(0, len(reachable), max(1, args.batch)):
                idx = reachable[b:b + max(1, args.batch)]
                _, fg, known = pwcnet_amd.plate_difference(torch.from_numpy(np.stack([frames[i] for i in idx])).cuda(), plate, count,
                                                           to_canvas[idx], args.plate_foreground, **proj)
                shown = torch.where(known, fg.to(torch.uint8) * 255, torch.full_like(fg, 128, dtype=torch.uint8)).cpu().numpy()
                for k, i in enumerate(idx):
                    dname, fname = out_stem(paths[i])
                    os.makedirs(os.path.join(args.out, dname), exist_ok=True)
                    Image.fromarray(shown[k]).save(os.path.join(args.out, dname, fname + "_fg.png"))
    print("Figure saved")


if __name__ == "__main__":
    main()

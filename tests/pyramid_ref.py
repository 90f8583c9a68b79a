"""The yardstick of the frame and mask pyramids (csrc/pwc_pyramid.hip, pwcnet_amd/pyramid.py), float64 torch on the CPU, and the
inputs the GPU tests use.  tests/test_host_pyramid.py validates it (hand-computed cases, avg_pool2d in float64, the order
independence of byte sums); tests/test_gpu_pyramid.py holds the kernel to it.

    frame_pyramid_ref(frames, factors)            a reshape to blocks, .double().sum() and a division, rounded to float32 once;
                                                  uint8 goes through v.float() / 255 first (the float32 nearest v / 255)
    mask_pyramid_ref(valid, factors, min_fraction)  integer counts of the non-zero bytes per block, mask = count >= need
"""
import functools
import math

import numpy as np
import torch

DEFAULT = (64, 32, 16, 8, 4)

# (N, H, W, C), factors -- the smallest shapes at which the indexing can still go wrong: more than one image, one block per image,
# a 1 x 1 coarsest level, four channels, a tile count that is no power of two, a single level, levels that are not asked for in
# between, the order asked, and a largest factor below 16 (frames narrower than a lane's 16-pixel piece: the narrow loads)
FRAME_CASES = {
    "n2_64x128x3": ((2, 64, 128, 3), DEFAULT),
    "64x64x1": ((1, 64, 64, 1), DEFAULT),
    "128x64x4": ((1, 128, 64, 4), DEFAULT),
    "192x320x3": ((1, 192, 320, 3), DEFAULT),
    "only2": ((2, 64, 128, 3), (2,)),
    "f8_32": ((2, 64, 128, 3), (8, 32)),
    "f32_8": ((2, 64, 128, 3), (32, 8)),
    "16x24_f8_2": ((1, 16, 24, 3), (8, 2)),
    # 32 x 125 blocks of 4 x 4: enough of them (two workgroups per compute unit of a 256-unit device) that a workgroup's tile
    # is eight blocks wide, and the last tile of a row only five
    "64x500_f4_2": ((2, 64, 500, 3), (4, 2)),
}
MIN_FRACTIONS = (1.0, 0.5, 1.0 / 4096)
DENSITIES = (0.1, 0.5, 0.9)


def _seed(name, salt=0):
    return (sum(ord(c) * (i + 1) for i, c in enumerate(name)) + 7919 * salt) % (2 ** 31)


def to_float(frames):
    """What a frame element enters the sums as: float32, a byte v as the float32 nearest v / 255."""
    return frames.float() / 255 if frames.dtype == torch.uint8 else frames


def block_sums(x, f):
    """(N, H/f, W/f, C) float64 (int64 for integer x) sums of the f x f blocks of x (N, H, W, C)."""
    N, H, W, C = x.shape
    return x.reshape(N, H // f, f, W // f, f, C).sum(dim=(2, 4))


def frame_pyramid_ref(frames, factors=DEFAULT):
    x = to_float(frames).double()
    return [(block_sums(x, f) / float(f * f)).float() for f in factors]


def need_ref(f, min_fraction):
    return max(1, math.ceil(min_fraction * f * f))


def mask_pyramid_ref(valid, factors=DEFAULT, min_fraction=1.0):
    """(masks, counts): torch.bool and torch.int32 (N, H/f, W/f) per factor."""
    v = (valid != 0).to(torch.int64)[..., None]
    counts = [block_sums(v, f)[..., 0].to(torch.int32) for f in factors]
    return [c >= need_ref(f, min_fraction) for c, f in zip(counts, factors)], counts


@functools.lru_cache(maxsize=None)
def byte_frames(name):
    shape, _ = FRAME_CASES[name]
    return torch.from_numpy(np.random.RandomState(_seed(name)).randint(0, 256, size=shape).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def byte_ref(name):
    """The reference pyramid of byte_frames(name), computed once and shared; do not write to it."""
    return frame_pyramid_ref(byte_frames(name), FRAME_CASES[name][1])


@functools.lru_cache(maxsize=None)
def dyadic_frames(name):
    """float32 multiples of 2^-16 in [0, 1): a 64 x 64 block sums to below 2^12 in steps of 2^-16 -- 28 bits, exact in double in
    any order, and not in a float32 accumulator."""
    shape, _ = FRAME_CASES[name]
    k = np.random.RandomState(_seed(name, 1)).randint(0, 1 << 16, size=shape)
    return torch.from_numpy((k.astype(np.float64) / 65536.0).astype(np.float32))


@functools.lru_cache(maxsize=None)
def positive_frames(name):
    """Non-negative float32 with magnitudes from 2^-20 to 1."""
    shape, _ = FRAME_CASES[name]
    e = np.random.RandomState(_seed(name, 2)).uniform(-20.0, 0.0, size=shape)
    return torch.from_numpy(np.exp2(e).astype(np.float32))


@functools.lru_cache(maxsize=None)
def signed_frames(name):
    x = positive_frames(name)
    s = np.random.RandomState(_seed(name, 3)).randint(0, 2, size=tuple(x.shape)) * 2 - 1
    return x * torch.from_numpy(s.astype(np.float32))


@functools.lru_cache(maxsize=None)
def random_mask(name, density):
    (N, H, W, _), _ = FRAME_CASES[name]
    return torch.from_numpy(np.random.RandomState(_seed(name, 4 + int(density * 10))).uniform(size=(N, H, W)) < density)

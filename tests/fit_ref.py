"""Yardstick of the frame fit and the flow refit (pwcnet_amd/fit.py, csrc/pwc_fit.hip): their arithmetic restated in numpy.  Run
in float64 (the default) it is the reference, unrounded; run with dtype=np.float32 every step of it -- the sample coordinate,
the weights, the blend, the refit scale -- is float32 arithmetic, the planted fault that shows the tests' bound can tell "formed
in double, rounded once" from a straightforward float32 composition.  Not a test file; tests/test_host_fit.py validates it
without a GPU, tests/test_gpu_fit.py holds the kernels to it.

Per axis (`inn` source samples, `out` output samples, output index d), half-pixel centres:
    src = ((2 d + 1) inn - out) / (2 out)      one division of exact integers, clamped to [0, inn - 1]
    i0 = floor(src), f = src - i0, i1 = min(i0 + 1, inn - 1)
value = (1 - fy) ((1 - fx) a + fx b) + fy ((1 - fx) c + fx d) over the corners a = (y0, x0), b = (y0, x1), c = (y1, x0),
d = (y1, x1); the refit multiplies it by W / FW (u) or H / FH (v).  Mode "pad": fit repeats the last row and column, refit crops.
"""
import numpy as np

MODES = ("resize", "pad")

# N, (H, W) -> (OH, OW): the smallest sizes that reach each edge of the kernels
GEOMETRIES = [
    (1, 1, 1, 64, 64),           # every sample clamped
    (2, 65, 67, 128, 128),       # odd rows, unaligned uint8 rows, batch stride
    (1, 63, 130, 64, 192),
    (1, 64, 100, 64, 128),       # the exact-copy axis (H)
    (2, 127, 129, 128, 192),
    (1, 128, 192, 128, 192),     # already fits: the input object itself comes back
]


def ceil_to(n, factor=64):
    return -(-int(n) // factor) * factor


def taps(inn, out, dtype=np.float64):
    """(i0, i1, f) of every output index of one axis; f in `dtype`."""
    d = np.arange(out, dtype=np.int64)
    num, den = (2 * d + 1) * inn - out, 2 * out
    src = num.astype(dtype) / dtype(den)
    src = np.clip(src, dtype(0), dtype(inn - 1))
    fl = np.floor(src)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, inn - 1), (src - fl).astype(dtype)


def to_float32(images):
    """uint8 frames as the float32 the kernel reads them as, float(double(v) / 255.0); float32 frames as they are."""
    if images.dtype == np.uint8:
        return (images.astype(np.float64) / 255.0).astype(np.float32)
    assert images.dtype == np.float32, images.dtype
    return images


def resize(x, OH, OW, dtype=np.float64):
    """Half-pixel bilinear resize of (N, H, W, C) `x` to (N, OH, OW, C) in `dtype`, NOT rounded to float32.  Returns
    (value, S): S the largest magnitude among the four corners of every element."""
    x = x.astype(dtype)
    H, W = x.shape[1:3]
    y0, y1, fy = taps(H, OH, dtype)
    x0, x1, fx = taps(W, OW, dtype)
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    fy, fx = fy.reshape(1, OH, 1, 1), fx.reshape(1, 1, OW, 1)
    one = dtype(1)
    v = (one - fy) * ((one - fx) * a + fx * b) + fy * ((one - fx) * c + fx * d)
    S = np.maximum(np.maximum(np.abs(a), np.abs(b)), np.maximum(np.abs(c), np.abs(d))).astype(np.float64)
    assert v.dtype == dtype
    return v, S


def fit_frames(images, mode="resize", factor=64, dtype=np.float64):
    """(N, H, W, 3) uint8 / float32 frames -> (value, S) at (N, ceil(H), ceil(W), 3), value unrounded in `dtype`."""
    assert mode in MODES
    x = to_float32(images)
    H, W = x.shape[1:3]
    OH, OW = ceil_to(H, factor), ceil_to(W, factor)
    if mode == "pad":
        v = x[:, np.minimum(np.arange(OH), H - 1)][:, :, np.minimum(np.arange(OW), W - 1)].astype(dtype)
        return v, np.abs(v).astype(np.float64)
    return resize(x, OH, OW, dtype)


def refit_flow(flow, H, W, mode="resize", dtype=np.float64):
    """(N, FH, FW, 2) float32 flow at network geometry -> (value, S) at (N, H, W, 2): resized and scaled by (W / FW, H / FH), or
    cropped.  S is the corners' largest magnitude times the scale."""
    assert mode in MODES and flow.dtype == np.float32
    FH, FW = flow.shape[1:3]
    if mode == "pad":
        assert FH >= H and FW >= W
        v = flow[:, :H, :W].astype(dtype)
        return v, np.abs(v).astype(np.float64)
    v, S = resize(flow, H, W, dtype)
    scale = np.array([dtype(W) / dtype(FW), dtype(H) / dtype(FH)], dtype=dtype)
    v = v * scale
    assert v.dtype == dtype
    return v, S * scale.astype(np.float64)


def ratio(y, ref, S):
    """Per element |y - ref| / (2^-24 S): at most 1 (plus the reference's own double rounding) for a float32 `y` that is the
    once-rounded value of a number no larger than S -- half an ulp of it.  Where S is 0 the value must be exactly 0."""
    err = np.abs(y.astype(np.float64) - ref.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / (2.0 ** -24 * S)
    return np.where(S == 0, np.where(err == 0, 0.0, np.inf), r)


BOUND = 1.0 + 1e-6      # half an ulp, and the reference's own double rounding

"""Pins the conv routing: which C entry points every layer of the supported configurations calls, with which scalar
arguments and in which order.

The capture swaps the loaded library handle for a thin proxy.  Every entry point whose name ends in `_f32` is recorded as
(name, arguments) -- ints and floats as they are, pointers only as null / non-null -- and then called.  Host queries
(`*_supported`, `*_plan`, `*_floats`) are not recorded.  Model scenarios also record the model's launch plans as
(what, kernel name, flops, bytes, executed flops): bench.py's roofline and the profiler tables key on them.

The fixture (tests/golden/conv_dispatch.json.gz) is written by tests/golden/make_dispatch_golden.py.
"""
import ctypes
import gzip
import json
import os

import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch.json.gz")

# name -> (kind, batch, height, width, constructor kwargs)
SCENARIOS = {
    "b8_448x1024": ("model", 8, 448, 1024, {}),
    "b8_448x1024_dc": ("model", 8, 448, 1024, {"use_dc": True}),
    "b8_448x1024_track_max": ("model", 8, 448, 1024, {"track_max": True}),
    "b8_448x1024_fp32": ("model", 8, 448, 1024, {"f16x2": False}),
    "b8_448x1024_fp32_no_wino4": ("model", 8, 448, 1024, {"f16x2": False, "winograd4": False}),
    "b8_448x1024_fp32_no_wino": ("model", 8, 448, 1024, {"f16x2": False, "winograd": False}),
    "b1_448x1024": ("model", 1, 448, 1024, {}),
    "b8_960x1920": ("model", 8, 960, 1920, {}),
    "b2_64x128": ("model", 2, 64, 128, {}),
    "b2_64x128_dc": ("model", 2, 64, 128, {"use_dc": True}),
    "seq9_448x1024": ("sequence", 9, 448, 1024, {}),
    "train_b2_64x128": ("train", 2, 64, 128, {}),
    "train_b4_384x448": ("train", 4, 384, 448, {}),
}


class _Recorder:
    """Stands in for the loaded ctypes handle: records every `_f32` call, passes everything else through."""

    def __init__(self, handle):
        self._handle = handle
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._handle, name)
        if not name.endswith("_f32"):
            return fn
        calls = self.calls

        def call(*args):
            rec = []
            for a, t in zip(args, fn.argtypes):
                if t is ctypes.c_void_p:
                    rec.append("null" if not (a.value if isinstance(a, ctypes.c_void_p) else a) else "ptr")
                elif t is ctypes.c_float:
                    rec.append(float(a))
                else:
                    rec.append(int(a))
            calls.append([name, rec])
            return fn(*args)

        call.argtypes = fn.argtypes
        return call


def _reset_workspaces():
    from pwcnet_amd import grad_ops, modules
    modules._WS.clear()
    modules._H2_WS.clear()
    grad_ops._WS.clear()
    grad_ops._WARP_WS.clear()


def capture(name, monkeypatch):
    """Runs one scenario on a fresh model / trainer and returns {"calls": [...], "plans": [...]}."""
    import pwcnet_amd
    from pwcnet_amd import _lib
    kind, n, h, w, kw = SCENARIOS[name]
    dev = torch.device("cuda")
    torch.manual_seed(0)
    torch.cuda.synchronize()
    _reset_workspaces()
    rec = _Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "_lib", rec)
    plans = []
    if kind == "train":
        from pwcnet_amd.train import Trainer
        tn = Trainer(**kw)
        tn.load_weights(util.model_weights(False))
        im0, im1 = util.smooth_images(n, h, w)
        gt = util.flow_field(n, h, w)
        tn.step(torch.from_numpy(im0).to(dev), torch.from_numpy(im1).to(dev), torch.from_numpy(gt).to(dev))
    else:
        net = pwcnet_amd.PWCDCNet(**kw)
        net.load_weights(util.model_weights(kw.get("use_dc", False)))
        if kind == "sequence":
            frames = torch.from_numpy(util.smooth_images(n, h, w)[0]).to(dev)
            net(frames[:-1], frames[1:])
        else:
            # both batches in one buffer, one frame apart: images_1 never lands right behind images_0 (at batch 1 that would
            # be the sequence form, whichever way the allocator placed them)
            im0, im1 = util.smooth_images(n, h, w)
            frames = torch.empty((2 * n + 1, h, w, 3), dtype=torch.float32, device=dev)
            frames[:n], frames[n + 1:] = torch.from_numpy(im0), torch.from_numpy(im1)
            net(frames[:n], frames[n + 1:])
        for plan in net._plans.values():
            plans.append([[what, kname, flops, nbytes, xflops] for _, _, what, kname, flops, nbytes, xflops in plan.calls])
    torch.cuda.synchronize()
    monkeypatch.undo()
    return {"calls": rec.calls, "plans": plans}


@pytest.fixture(scope="module")
def golden():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def _first_difference(got, exp):
    for i, (a, b) in enumerate(zip(got, exp)):
        if a != b:
            return f"entry {i}: got {a}, expected {b}"
    return f"lengths differ: got {len(got)}, expected {len(exp)}"


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_conv_dispatch_matches_recorded_trace(name, golden, monkeypatch):
    got = json.loads(json.dumps(capture(name, monkeypatch)))       # (the fixture's own number forms)
    exp = golden[name]
    assert got["calls"] == exp["calls"], f"{name}, C calls: " + _first_difference(got["calls"], exp["calls"])
    assert len(got["plans"]) == len(exp["plans"]), name
    for g, e in zip(got["plans"], exp["plans"]):
        assert g == e, f"{name}, launch plan: " + _first_difference(g, e)

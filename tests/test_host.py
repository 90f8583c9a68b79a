"""CPU tests of the host logic: C-ABI surface, variable inventory, channel layouts,
checkpoint bundle reader/writer, pair sharding (incl. a world-size-2 gloo run)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pwcnet_amd import _lib, ckpt, sharding
from pwcnet_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ C ABI
def test_library_exports_every_declared_symbol():
    """Every function include/pwc_hip.h declares is exported by the built .so and bound
    in _lib.SIGNATURES (no compute call is made: there is no GPU here)."""
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    declared = set(re.findall(r"\b(pwc_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    L = _lib.lib()
    for name in declared:
        assert hasattr(L, name)
    assert L.pwc_version() >= 100
    assert L.pwc_error_string(-1).decode().startswith("invalid argument")
    # pure host-side helpers are callable without a GPU
    assert L.pwc_conv3x3_packed_floats(160, 128) == 9 * 160 * 128
    plan = (ctypes.c_int * 4)()
    assert L.pwc_conv3x3_plan(8 * 112 * 256, 128, 160, plan) == 0
    bm, bn = ctypes.c_int(), ctypes.c_int()
    assert L.pwc_conv3x3_tile_shape(plan[0], bm, bn) == 0 and (bm.value, bn.value) == (128, 128)
    assert plan[1] == -1 and plan[2] == 8 * 112 * 256 and plan[3] == 1
    # mid-size M: the largest tile that still gives >= 384 workgroups (measured rule)
    assert L.pwc_conv3x3_plan(8 * 28 * 64, 128, 224, plan) == 0
    assert L.pwc_conv3x3_tile_shape(plan[0], bm, bn) == 0 and (bm.value, bn.value, plan[3]) == (32, 128, 1)
    assert L.pwc_conv3x3_plan(8 * 7 * 16, 128, 288, plan) == 0 and plan[3] in (3, 9)   # tiny M: tap split
    assert L.pwc_conv3x3_workspace_floats(100, 20) == 9 * 100 * 32
    # argument validation happens before any launch
    assert L.pwc_cost_volume_f32(None, 4, None, 4, None, 81, 1, 4, 4, 4, 4, 0.1, None) == -1
    assert L.pwc_conv3x3_f32(None, 16, None, None, None, 16, 1, 4, 4, 16, 16, 1, 1, 1, 0.1, -1, 0, None, 0, None) == -1


def test_hot_kernels_do_not_spill_to_scratch(tmp_path):
    """A regression guard that needs no GPU (round 6: a third buffer resource in conv3x3_h2_kernel took six more SGPRs, the
    128-cout variants went over 256 VGPRs into scratch and every launch ran 2 x slower -- green tests, half the throughput).
    The code objects inside the built libpwc_hip.so say what each kernel takes: the matrix-pipe kernels that carry the forward
    must have NO private segment (scratch); the C = 96 correlation variants are allowed their few spilled registers."""
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf of the ROCm toolchain not found")
    _lib.lib()
    import shutil
    so = shutil.copy(_lib.LIB_PATH, str(tmp_path / "lib.so"))
    subprocess.check_call([objdump, "--offloading", so], cwd=str(tmp_path), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    scratch = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", str(tmp_path / f)], capture_output=True, text=True).stdout
        name = None
        for line in notes.splitlines():
            line = line.strip()
            if line.startswith(".name:"):
                name = line.split(":", 1)[1].strip()
            elif line.startswith(".private_segment_fixed_size:") and name:
                scratch[name] = int(line.split(":", 1)[1])
                name = None
    hot = [k for k in scratch if re.search(r"conv3x3_(h2|w32|t32|sk|skp|c16pair)_kernel|cost_volume_(h2|blk)_kernel", k)]
    assert len(hot) >= 30, sorted(scratch)
    bad = {k: v for k, v in scratch.items() if k in hot and v > (48 if "cost_volume_h2_kernelILi6" in k else 0)}
    assert not bad, bad


def test_production_library_has_no_debug_knobs():
    """VERDICT r5 item 5 / SURVEY 8(b) "no global mutable state": the production libpwc_hip.so exports no pwc_debug_* symbol
    (the tile-pinning / ablation knobs of the A/B scripts live in libpwc_hip_harness.so, built with -DPWC_HARNESS only when a
    script asks, PWC_HARNESS=1), the header declares none, and the tile of the small-launch conv is an ARGUMENT
    (pwc_conv3x3_sk_variant_f32) validated before any launch."""
    assert not _lib.HARNESS and _lib.LIB_PATH.endswith("libpwc_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [ln.split()[-1] for ln in out.splitlines() if ln.strip()]
    assert any(n == "pwc_version" for n in exported)
    assert [n for n in exported if "debug" in n.lower()] == []
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert not re.search(r"\bpwc_debug_[a-z0-9_]+\s*\(", header)
    assert not any("debug" in n for n in _lib.SIGNATURES)
    L = _lib.lib()
    for name in _lib.HARNESS_SIGNATURES_NAMES:
        assert not hasattr(L, name), name
    al = ctypes.c_void_p(4096)      # (an aligned non-null address: argument checks only, nothing is launched)
    v = L.pwc_conv3x3_sk_variant_f32
    assert v(al, 64, al, al, al, 32, 1, 8, 8, 64, 32, 1, 1, 1, 0.1, 0, None) == -1       # tile 0 is pwc_conv3x3_sk_f32's business
    assert v(al, 64, al, al, al, 32, 1, 8, 8, 64, 32, 1, 1, 1, 0.1, 13, None) == -1      # no such tile
    assert v(al, 64, al, al, al, 48, 1, 8, 8, 64, 48, 1, 1, 1, 0.1, 22, None) == -4      # x2 tiles need Cout % 32 == 0
    assert v(al, 64, al, al, al, 32, 1, 8, 8, 64, 32, 1, 2, 1, 0.1, 31, None) == -4      # the LDS-patch form takes no dilation
    assert v(al, 320, al, al, al, 32, 1, 8, 8, 320, 32, 1, 1, 1, 0.1, 41, None) == -4    # ... and at most 288 input channels


_AL, _MIS = 4096, 4100      # an aligned and a 4-byte-aligned-only non-null address: argument checks only, nothing is launched
_EINVAL, _EALIGN, _ERANGE, _EUNSUP = -1, -2, -3, -4
# entry point -> (argument names in call order, a call that passes every check)
_F16_CONV_CALLS = {
    "pwc_conv3x3_h2_f32": (
        "x x_cs pw bias y y_cs N H W Cin Cout dil act slope ws wsf stream",
        dict(x=_AL, x_cs=64, pw=_AL, bias=_AL, y=_AL, y_cs=64, N=1, H=16, W=32, Cin=64, Cout=64, dil=1, act=1, slope=0.1, ws=None, wsf=0, stream=None)),
    "pwc_conv3x3_h2_ex_f32": (
        "x x_cs Cin_a x2 x2_cs pw bias y y_cs N H W Cin Cout dil act slope ws wsf status stream",
        dict(x=_AL, x_cs=32, Cin_a=32, x2=_AL, x2_cs=32, pw=_AL, bias=_AL, y=_AL, y_cs=64, N=1, H=16, W=32, Cin=64, Cout=64, dil=1, act=1,
             slope=0.1, ws=None, wsf=0, status=None, stream=None)),
    "pwc_conv3x3_h2_ex3_f32": (
        "x x_cs Cin_a x2 x2_cs Cin_b x3 x3_cs pw bias y y_cs N H W Cin Cout act slope ws wsf status stream",
        dict(x=_AL, x_cs=84, Cin_a=96, x2=_AL, x2_cs=32, Cin_b=32, x3=_AL, x3_cs=32, pw=_AL, bias=_AL, y=_AL, y_cs=64, N=1, H=16, W=32,
             Cin=160, Cout=64, act=1, slope=0.1, ws=None, wsf=0, status=None, stream=None)),
    "pwc_conv3x3_h2_stride2_f32": (
        "x x_cs pw bias y y_cs N H W Cin Cout act slope ws wsf status stream",
        dict(x=_AL, x_cs=16, pw=_AL, bias=_AL, y=_AL, y_cs=32, N=1, H=16, W=32, Cin=16, Cout=32, act=1, slope=0.1, ws=None, wsf=0, status=None,
             stream=None)),
    "pwc_conv3x3_sk_f32": (
        "x x_cs pw bias y y_cs N H W Cin Cout stride dil act slope stream",
        dict(x=_AL, x_cs=64, pw=_AL, bias=_AL, y=_AL, y_cs=32, N=1, H=16, W=32, Cin=64, Cout=32, stride=1, dil=1, act=1, slope=0.1, stream=None)),
    "pwc_conv3x3_t32_f32": (
        "x x_cs pw bias y y_cs N H W Cin Cout stride act slope stream",
        dict(x=_AL, x_cs=16, pw=_AL, bias=_AL, y=_AL, y_cs=32, N=1, H=16, W=32, Cin=16, Cout=32, stride=1, act=1, slope=0.1, stream=None)),
    "pwc_conv3x3_w32_f32": (
        "x x_cs pw bias y y_cs N H W Cin Cout act slope stream",
        dict(x=_AL, x_cs=32, pw=_AL, bias=_AL, y=_AL, y_cs=32, N=1, H=16, W=32, Cin=32, Cout=32, act=1, slope=0.1, stream=None)),
    "pwc_conv3x3_c16pair_f32": (
        "x x_cs pw b1 b2 y y_cs N H W slope stream",
        dict(x=_AL, x_cs=16, pw=_AL, b1=_AL, b2=_AL, y=_AL, y_cs=16, N=1, H=16, W=32, slope=0.1, stream=None)),
    "pwc_conv3x3_c3c16pair_f32": (
        "x N x_b N_b pw b0 b1 b2 y y_cs H W slope stream",
        dict(x=_AL, N=1, x_b=None, N_b=0, pw=_AL, b0=_AL, b1=_AL, b2=_AL, y=_AL, y_cs=16, H=32, W=64, slope=0.1, stream=None)),
}
_BIG = dict(H=16384, W=16384)          # 2^28 pixels of one image: past every family's 32-bit byte range, the 3-channel frames' too
_OPERANDS_FIRST = ("pwc_conv3x3_h2_ex_f32", "pwc_conv3x3_h2_ex3_f32")      # the rules of operands 2 / 3 (their range too) come first
# (entry point, the bad arguments, the code): one fault per row first, then rows with two faults that pin which one is reported
_F16_CONV_FAULTS = [(name, bad, code) for name in _F16_CONV_CALLS for bad, code in (
    (dict(x=None), _EINVAL), (dict(pw=None), _EINVAL), (dict(y=None), _EINVAL),           # a null pointer
    (dict(N=0), _EINVAL), (dict(H=-1), _EINVAL),                                        # a non-positive size
    (dict(y_cs=12), _EINVAL),                                                           # a channel stride below the channel count
    (dict(y=_MIS), _EALIGN), (dict(pw=_MIS), _EALIGN),                                  # a misaligned pointer
    (dict(y_cs=66), _EALIGN),                                                           # a misaligned channel stride
    (dict(_BIG), _ERANGE),                                                              # a shape past the 32-bit range
    (dict(x=None, y=_MIS), _EINVAL), (dict(y_cs=12, y=_MIS), _EINVAL),
    (dict(_BIG, y=_MIS), _ERANGE if name in _OPERANDS_FIRST else _EALIGN), (dict(_BIG, N=0), _ERANGE if name in _OPERANDS_FIRST else _EINVAL))] + [
    ("pwc_conv3x3_h2_f32", dict(bias=None), _EINVAL), ("pwc_conv3x3_h2_f32", dict(W=0), _EINVAL), ("pwc_conv3x3_h2_f32", dict(dil=0), _EINVAL),
    ("pwc_conv3x3_h2_f32", dict(x_cs=48), _EINVAL), ("pwc_conv3x3_h2_f32", dict(x=_MIS), _EALIGN), ("pwc_conv3x3_h2_f32", dict(bias=_MIS), _EALIGN),
    ("pwc_conv3x3_h2_f32", dict(ws=_MIS), _EALIGN), ("pwc_conv3x3_h2_f32", dict(x_cs=66), _EALIGN),
    ("pwc_conv3x3_h2_f32", dict(Cout=48), _EUNSUP), ("pwc_conv3x3_h2_f32", dict(Cin=24), _EUNSUP), ("pwc_conv3x3_h2_f32", dict(Cout=1024, y_cs=1024), _EUNSUP),
    ("pwc_conv3x3_h2_f32", dict(Cin=0), _EINVAL), ("pwc_conv3x3_h2_f32", dict(Cin=-16), _EINVAL),
    ("pwc_conv3x3_h2_f32", dict(dil=0, Cout=48), _EINVAL), ("pwc_conv3x3_h2_f32", dict(Cout=48, y_cs=32), _EUNSUP),
    ("pwc_conv3x3_h2_f32", dict(Cin=24, x_cs=16), _EUNSUP), ("pwc_conv3x3_h2_f32", dict(_BIG, ws=_MIS), _EALIGN),
    ("pwc_conv3x3_h2_ex_f32", dict(x2=_MIS, N=0), _EALIGN), ("pwc_conv3x3_h2_ex_f32", dict(status=_MIS, N=0), _EALIGN),
    ("pwc_conv3x3_h2_ex_f32", dict(x_cs=16), _EINVAL), ("pwc_conv3x3_h2_ex_f32", dict(x2_cs=16), _EINVAL), ("pwc_conv3x3_h2_ex_f32", dict(Cin_a=24), _EINVAL),
    ("pwc_conv3x3_h2_ex_f32", dict(Cin_a=64), _EINVAL), ("pwc_conv3x3_h2_ex_f32", dict(x2_cs=34), _EALIGN), ("pwc_conv3x3_h2_ex_f32", dict(Cout=48), _EUNSUP),
    ("pwc_conv3x3_h2_ex_f32", dict(x2=None, x_cs=32), _EINVAL), ("pwc_conv3x3_h2_ex_f32", dict(x_cs=34), _EALIGN), ("pwc_conv3x3_h2_ex_f32", dict(Cin=72, x2_cs=40), _EUNSUP),
    ("pwc_conv3x3_h2_ex3_f32", dict(x3=None), _EINVAL), ("pwc_conv3x3_h2_ex3_f32", dict(x_cs=80), _EINVAL), ("pwc_conv3x3_h2_ex3_f32", dict(x3_cs=16), _EINVAL),
    ("pwc_conv3x3_h2_ex3_f32", dict(Cin_b=24), _EINVAL), ("pwc_conv3x3_h2_ex3_f32", dict(x3=_MIS, Cout=48), _EALIGN), ("pwc_conv3x3_h2_ex3_f32", dict(Cout=48), _EUNSUP),
    ("pwc_conv3x3_h2_ex3_f32", dict(x_cs=86), _EALIGN),
    ("pwc_conv3x3_h2_stride2_f32", dict(H=15), _EUNSUP), ("pwc_conv3x3_h2_stride2_f32", dict(Cout=48, y_cs=48), _EUNSUP),
    ("pwc_conv3x3_h2_stride2_f32", dict(H=15, x_cs=12), _EUNSUP), ("pwc_conv3x3_h2_stride2_f32", dict(x_cs=12), _EINVAL),
    ("pwc_conv3x3_sk_f32", dict(bias=None), _EINVAL), ("pwc_conv3x3_sk_f32", dict(stride=3), _EINVAL), ("pwc_conv3x3_sk_f32", dict(dil=0), _EINVAL),
    ("pwc_conv3x3_sk_f32", dict(x_cs=32), _EINVAL), ("pwc_conv3x3_sk_f32", dict(x=_MIS), _EALIGN), ("pwc_conv3x3_sk_f32", dict(x_cs=66), _EALIGN),
    ("pwc_conv3x3_sk_f32", dict(Cin=48), _EUNSUP), ("pwc_conv3x3_sk_f32", dict(Cout=24), _EUNSUP), ("pwc_conv3x3_sk_f32", dict(Cin=-5), _EINVAL),
    ("pwc_conv3x3_sk_f32", dict(N=8, H=1024, W=1024), _ERANGE), ("pwc_conv3x3_sk_f32", dict(Cin=48, x_cs=32), _EUNSUP),
    ("pwc_conv3x3_sk_f32", dict(stride=3, Cin=48), _EINVAL), ("pwc_conv3x3_sk_f32", dict(N=8, H=1024, W=1024, bias=_MIS), _EALIGN),
    ("pwc_conv3x3_t32_f32", dict(stride=0), _EINVAL), ("pwc_conv3x3_t32_f32", dict(Cin=24, x_cs=32), _EUNSUP), ("pwc_conv3x3_t32_f32", dict(Cout=64, y_cs=64), _EUNSUP),
    ("pwc_conv3x3_t32_f32", dict(Cin=32, x_cs=32, stride=2), _EUNSUP), ("pwc_conv3x3_t32_f32", dict(stride=3, Cin=24), _EINVAL),
    ("pwc_conv3x3_t32_f32", dict(Cin=32, x_cs=16), _EINVAL), ("pwc_conv3x3_t32_f32", dict(x=_MIS), _EALIGN), ("pwc_conv3x3_t32_f32", dict(x_cs=18), _EALIGN),
    ("pwc_conv3x3_t32_f32", dict(N=32, H=1024, W=1024), _ERANGE), ("pwc_conv3x3_t32_f32", dict(N=16, H=1024, W=1024), _ERANGE),       # (the input's range, the output's)
    ("pwc_conv3x3_t32_f32", dict(N=16, H=1024, W=1024, bias=_MIS), _EALIGN),
    ("pwc_conv3x3_w32_f32", dict(Cin=16), _EUNSUP), ("pwc_conv3x3_w32_f32", dict(Cout=64, y_cs=64), _EUNSUP), ("pwc_conv3x3_w32_f32", dict(Cin=16, x=_MIS), _EUNSUP),
    ("pwc_conv3x3_w32_f32", dict(Cin=64), _EINVAL), ("pwc_conv3x3_w32_f32", dict(x_cs=34), _EALIGN), ("pwc_conv3x3_w32_f32", dict(N=16, H=1024, W=1024), _ERANGE),
    ("pwc_conv3x3_w32_f32", dict(N=8, H=1024, W=1024, y_cs=64), _ERANGE), ("pwc_conv3x3_w32_f32", dict(Cin=0), _EINVAL),
    ("pwc_conv3x3_c16pair_f32", dict(b2=None), _EINVAL), ("pwc_conv3x3_c16pair_f32", dict(b2=None, x=_MIS), _EINVAL), ("pwc_conv3x3_c16pair_f32", dict(b2=_MIS), _EALIGN),
    ("pwc_conv3x3_c16pair_f32", dict(_BIG, b2=_MIS), _EALIGN), ("pwc_conv3x3_c16pair_f32", dict(x_cs=12), _EINVAL), ("pwc_conv3x3_c16pair_f32", dict(x_cs=12, y=_MIS), _EINVAL),
    ("pwc_conv3x3_c16pair_f32", dict(x_cs=18), _EALIGN),
    ("pwc_conv3x3_c3c16pair_f32", dict(W=62), _EUNSUP), ("pwc_conv3x3_c3c16pair_f32", dict(N_b=1), _EINVAL), ("pwc_conv3x3_c3c16pair_f32", dict(N_b=-1), _EINVAL),
    ("pwc_conv3x3_c3c16pair_f32", dict(W=62, y=_MIS), _EUNSUP), ("pwc_conv3x3_c3c16pair_f32", dict(W=62, y_cs=12), _EINVAL), ("pwc_conv3x3_c3c16pair_f32", dict(b0=_MIS), _EALIGN),
]


def test_f16_conv_entry_points_report_the_same_codes():
    """The argument checks of the F16-matrix-pipe conv entry points (conv3x3_h2 / sk / t32 / w32 / c16pair) go through one shared
    checker (pwc_conv_io_check, pwc_common.h); every family keeps the checks that are its own.  This table pins which code each
    entry point returns for a bad call -- one fault at a time, then two at once (which one wins) -- as recorded from the
    library before the checks were shared.  Every row fails a check: nothing is launched, no GPU is needed."""
    L = _lib.lib()
    assert all(code != 0 for _, _, code in _F16_CONV_FAULTS)
    got = []
    for name, bad, code in _F16_CONV_FAULTS:
        names, good = _F16_CONV_CALLS[name]
        assert set(bad) <= set(good), (name, bad)
        args = dict(good, **bad)
        rc = getattr(L, name)(*[args[k] for k in names.split()])
        if rc != code:
            got.append((name, bad, code, rc))
    assert not got, got


_FP32_CONV_ARGS = "x x_cs pw bias y y_cs N H W Cin Cout dil act slope stream"
_FP32_CONV_GOOD = dict(x=_AL, x_cs=32, pw=_AL, bias=_AL, y=_AL, y_cs=32, N=1, H=16, W=32, Cin=32, Cout=32, dil=1, act=1, slope=0.1, stream=None)
_FP32_PACK_GOOD = dict(w=_AL, cmap=None, Cin=16, Cin_phys=16, Cout=16, packed=_AL, stream=None)
# entry point -> (argument names in call order, a call that passes every check)
_FP32_CONV_CALLS = {
    "pwc_conv3x3_f32": (
        "x x_cs pw bias y y_cs N H W Cin Cout stride dil act slope tile split ws wsf stream",
        dict(_FP32_CONV_GOOD, stride=1, tile=-1, split=0, ws=None, wsf=0)),
    "pwc_conv3x3_wino_f32": (_FP32_CONV_ARGS, _FP32_CONV_GOOD),
    "pwc_conv3x3_wino_split_f32": (
        "x x_cs pw bias y y_cs N H W Cin Cout dil act slope csplit ws wsf stream",
        dict(_FP32_CONV_GOOD, csplit=1, ws=_AL, wsf=2 * 16 * 32 * 32)),
    "pwc_conv3x3_wino4_f32": (_FP32_CONV_ARGS, _FP32_CONV_GOOD),
    "pwc_conv3x3_pack_f32": ("w cmap Cin Cin_phys Cout packed stream", _FP32_PACK_GOOD),
    "pwc_conv3x3_wino_pack_f32": ("w cmap Cin Cin_phys Cout packed stream", _FP32_PACK_GOOD),
    "pwc_conv3x3_wino4_pack_f32": ("w cmap Cin Cin_phys Cout packed stream", _FP32_PACK_GOOD),
}
_FP32_CONVS = tuple(n for n in _FP32_CONV_CALLS if "pack" not in n)
_FP32_PACKERS = tuple(n for n in _FP32_CONV_CALLS if "pack" in n)
_FP32_Y_ALIGNED = ("pwc_conv3x3_wino4_f32",)       # F(4x4) stores 16 bytes at a time; the others fall back to scalar stores
_FP32_WIDE = dict(_BIG, wsf=1 << 35)               # (a workspace long enough for the channel split's own check)
# (entry point, the bad arguments, the code): one fault per row first, then rows with two faults that pin which one is reported
_FP32_CONV_FAULTS = [(name, bad, code) for name in _FP32_CONVS for bad, code in (
    (dict(x=None), _EINVAL), (dict(pw=None), _EINVAL), (dict(bias=None), _EINVAL), (dict(y=None), _EINVAL),        # a null pointer
    (dict(N=0), _EINVAL), (dict(H=-1), _EINVAL), (dict(W=0), _EINVAL), (dict(Cin=0), _EINVAL), (dict(Cout=0), _EINVAL),     # a zero size
    (dict(dil=0), _EINVAL),
    (dict(Cin=24), _EUNSUP), (dict(Cout=24), _EUNSUP),                                  # channel counts that are no multiple of 16
    (dict(x_cs=16), _EINVAL), (dict(y_cs=16), _EINVAL),                                 # a channel stride below the channel count
    (dict(x=_MIS), _EALIGN), (dict(pw=_MIS), _EALIGN), (dict(bias=_MIS), _EALIGN), (dict(Cin=16, x_cs=18), _EALIGN),
    # a misaligned y or y_cs: F(4x4) refuses it, the others go on to their next rule (a short x_cs is reported first by all)
    (dict(y=_MIS, x_cs=16), _EINVAL), (dict(_FP32_WIDE, y=_MIS), _EALIGN if name in _FP32_Y_ALIGNED else _ERANGE),
    (dict(_FP32_WIDE, y_cs=34), _EALIGN if name in _FP32_Y_ALIGNED else _ERANGE),
    (dict(_FP32_WIDE), _ERANGE),                                                        # an image beyond 2^31 bytes
    # two faults of adjacent rules: null pointer / size, size / channel multiple, channel multiple / short stride,
    # short stride / alignment, alignment / range
    (dict(x=None, N=0), _EINVAL), (dict(x=None, Cin=24), _EINVAL), (dict(N=0, Cin=24), _EINVAL), (dict(dil=0, Cout=24), _EINVAL),
    (dict(Cin=24, x_cs=16), _EUNSUP), (dict(Cout=24, y_cs=16), _EUNSUP), (dict(Cin=24, x=_MIS), _EUNSUP),
    (dict(x_cs=16, x=_MIS), _EINVAL), (dict(y_cs=16, bias=_MIS), _EINVAL),
    (dict(_FP32_WIDE, x=_MIS), _EALIGN), (dict(_FP32_WIDE, pw=_MIS), _EALIGN), (dict(_FP32_WIDE, N=0), _EINVAL),
    (dict(_FP32_WIDE, Cin=24), _EUNSUP), (dict(_FP32_WIDE, y_cs=16), _EINVAL))] + [
    # the MFMA kernel's own: stride, tile, tap split and its workspace (the split is checked in front of the range, the tile
    # and the workspace behind it)
    ("pwc_conv3x3_f32", dict(stride=3), _EINVAL), ("pwc_conv3x3_f32", dict(stride=0), _EINVAL), ("pwc_conv3x3_f32", dict(stride=3, Cin=24), _EINVAL),
    ("pwc_conv3x3_f32", dict(split=2), _EINVAL), ("pwc_conv3x3_f32", dict(split=-1), _EINVAL), ("pwc_conv3x3_f32", dict(split=27), _EINVAL),
    ("pwc_conv3x3_f32", dict(split=2, x=_MIS), _EALIGN), ("pwc_conv3x3_f32", dict(_BIG, split=2), _EINVAL),
    ("pwc_conv3x3_f32", dict(tile=15), _EINVAL), ("pwc_conv3x3_f32", dict(tile=0), _EINVAL), ("pwc_conv3x3_f32", dict(_BIG, tile=15), _ERANGE),
    ("pwc_conv3x3_f32", dict(tile=14, split=3), _EINVAL), ("pwc_conv3x3_f32", dict(tile=14, split=3, ws=_MIS, wsf=1 << 20), _EINVAL),
    ("pwc_conv3x3_f32", dict(tile=14, split=3, ws=_AL, wsf=3 * 512 * 32 - 1), _EINVAL), ("pwc_conv3x3_f32", dict(split=9, ws=_AL, wsf=100), _EINVAL),
    ("pwc_conv3x3_f32", dict(N=1 << 12, H=1 << 10, W=1 << 9), _ERANGE),                 # 2^31 output pixels, each image in range
    # the channel split's own: csplit, its workspace -- reported in front of every shared rule
    ("pwc_conv3x3_wino_split_f32", dict(csplit=0), _EINVAL), ("pwc_conv3x3_wino_split_f32", dict(csplit=-2), _EINVAL),
    ("pwc_conv3x3_wino_split_f32", dict(csplit=3), _EINVAL), ("pwc_conv3x3_wino_split_f32", dict(csplit=2, ws=None), _EINVAL),
    ("pwc_conv3x3_wino_split_f32", dict(csplit=2, ws=_MIS), _EINVAL), ("pwc_conv3x3_wino_split_f32", dict(csplit=2, wsf=2 * 16 * 32 * 32 - 1), _EINVAL),
    ("pwc_conv3x3_wino_split_f32", dict(csplit=0, x=_MIS), _EINVAL), ("pwc_conv3x3_wino_split_f32", dict(csplit=2, ws=None, x=_MIS), _EINVAL),
    ("pwc_conv3x3_wino_split_f32", dict(csplit=2, ws=None, Cout=24), _EINVAL), ("pwc_conv3x3_wino_split_f32", dict(_BIG, csplit=2), _EINVAL),
    ("pwc_conv3x3_wino_split_f32", dict(csplit=2, Cin=24), _EINVAL), ("pwc_conv3x3_wino_split_f32", dict(csplit=2, x=_MIS), _EALIGN),
    ("pwc_conv3x3_wino_split_f32", dict(csplit=2, Cout=24), _EUNSUP), ("pwc_conv3x3_wino_split_f32", dict(_FP32_WIDE, csplit=2), _ERANGE)] + [
    # the packed weights behind one buffer resource: the two Winograd families only
    (name, dict(Cin=8192, x_cs=8192, Cout=4096, y_cs=4096, wsf=1 << 35), _ERANGE)
    for name in ("pwc_conv3x3_wino_f32", "pwc_conv3x3_wino_split_f32", "pwc_conv3x3_wino4_f32")] + [
    ("pwc_conv3x3_wino_f32", dict(Cin=8192, x_cs=8192, Cout=4096, y_cs=4096, x=_MIS), _EALIGN),
    ("pwc_conv3x3_wino4_f32", dict(Cin=8192, x_cs=8192, Cout=4096, y_cs=4096, y=_MIS), _EALIGN),
    ("pwc_conv3x3_wino4_f32", dict(y=_MIS), _EALIGN), ("pwc_conv3x3_wino4_f32", dict(y_cs=34), _EALIGN), ("pwc_conv3x3_wino4_f32", dict(y_cs=34, x_cs=16), _EINVAL),
    ("pwc_conv3x3_wino4_f32", dict(y=_MIS, Cout=24), _EUNSUP)] + [
    (name, bad, code) for name in _FP32_PACKERS for bad, code in (
        (dict(w=None), _EINVAL), (dict(packed=None), _EINVAL), (dict(Cin=0), _EINVAL), (dict(Cout=0), _EINVAL), (dict(Cout=-16), _EINVAL),
        (dict(Cin_phys=8), _EINVAL), (dict(Cin=24), _EINVAL),                           # fewer physical than logical channels
        (dict(Cin=8, Cin_phys=8), _EALIGN), (dict(Cin_phys=24), _EALIGN),               # physical channels in whole groups of 16
        (dict(w=None, Cin_phys=24), _EINVAL), (dict(Cin=24, Cin_phys=20), _EINVAL))]


def test_fp32_conv_entry_points_report_the_same_codes():
    """The argument checks of the fp32-matrix-pipe conv entry points (conv3x3_mfma / wino / wino4) and of their weight packers go
    through shared checkers (pwc_conv_io_check, pwc_common.h; the packers' in conv_fp32_common.h); every family keeps the rules
    that are its own (stride, tile, tap split, channel split, the ranges of its buffer resources, whether y must be aligned).
    This table pins which code each entry point returns for a bad call -- one fault at a time, then two at once (which one wins) --
    as recorded from the library before the checks were shared.  Every row fails a check: nothing is launched, no GPU is needed."""
    L = _lib.lib()
    assert all(code != 0 for _, _, code in _FP32_CONV_FAULTS)
    assert {name for name, _, _ in _FP32_CONV_FAULTS} == set(_FP32_CONV_CALLS)
    got = []
    for name, bad, code in _FP32_CONV_FAULTS:
        names, good = _FP32_CONV_CALLS[name]
        assert set(bad) <= set(good) | {"wsf"}, (name, bad)
        args = dict(good, **{k: v for k, v in bad.items() if k in good})                # (wsf: the entry points with a workspace)
        assert args != good, (name, bad)
        rc = getattr(L, name)(*[args[k] for k in names.split()])
        if rc != code:
            got.append((name, bad, code, rc))
    assert not got, got
    # the packed sizes: positions x physical input channels x output channels in whole groups of 16; 0 for a bad call
    for name, positions in (("pwc_conv3x3", 9), ("pwc_conv3x3_wino", 16), ("pwc_conv3x3_wino4", 36)):
        floats = getattr(L, name + "_packed_floats")
        assert floats(48, 24) == positions * 48 * 32 and floats(16, 16) == positions * 256
        assert floats(0, 16) == 0 and floats(16, 0) == 0 and floats(-16, 16) == 0


_MIS2 = 4098                # not even 4-byte aligned: the flow operand of the buffer-resource kernels
_CV_CONCAT_ARGS = "f0 f0_cs f1 f1_cs flow flow_cs scale out out_cs pad copy copy_cs N H W C R slope stream"
_CV_GOOD = dict(f0=_AL, f0_cs=32, f1=_AL, f1_cs=32, flow=_AL, flow_cs=2, scale=1.25, out=_AL, out_cs=84, pad=0, copy=_AL, copy_cs=32,
                N=1, H=16, W=32, C=32, R=4, slope=0.1, stream=None)
_CV_C64 = dict(C=64, f0_cs=64, f1_cs=64, copy_cs=64)
# entry point -> (argument names in call order, what a call that passes every check changes in _CV_GOOD)
_CV_CALLS = {
    "pwc_cost_volume_f32": ("f0 f0_cs f1 f1_cs out out_cs N H W C R slope stream", {}),
    "pwc_warp_cost_volume_f32": ("f0 f0_cs f1 f1_cs flow flow_cs scale out out_cs N H W C R slope stream", {}),
    "pwc_cost_volume_coarse_f32": ("f0 f0_cs f1 f1_cs flow flow_cs scale out out_cs copy copy_cs N H W C R slope stream", {}),
    "pwc_warp_cost_volume_concat_f32": (_CV_CONCAT_ARGS, {}),
    "pwc_warp_cost_volume_concat_h2_f32": (_CV_CONCAT_ARGS, {}),
    "pwc_warp_cost_volume_concat_blk_f32": (_CV_CONCAT_ARGS, _CV_C64),
}
_CV_CONCAT = tuple(n for n in _CV_CALLS if "concat" in n)
_CV_COPY = _CV_CONCAT + ("pwc_cost_volume_coarse_f32",)                       # entry points with the f0 concat copy
_CV_WIDE = dict(H=2048, W=2048)        # 2^22 pixels: a 128-float channel stride is past 2^31 bytes, the 84-float records are not
# (entry point, the bad arguments, the code): one fault per row first, then rows with two faults that pin which one is reported
_CV_FAULTS = [(name, bad, code) for name in _CV_CALLS for bad, code in (
    (dict(f0=None), _EINVAL), (dict(f1=None), _EINVAL), (dict(out=None), _EINVAL),      # a null pointer
    (dict(N=0), _EINVAL), (dict(H=-1), _EINVAL), (dict(W=0), _EINVAL), (dict(C=0), _EINVAL),    # a non-positive size
    (dict(R=0), _EUNSUP), (dict(R=5), _EUNSUP),                                         # the search range
    (dict(f0_cs=28), _EINVAL), (dict(f1_cs=28), _EINVAL), (dict(out_cs=80), _EINVAL),   # a channel stride below C, out_cs below 81
    (dict(C=30), _EALIGN), (dict(f0=_MIS), _EALIGN), (dict(f1=_MIS), _EALIGN), (dict(f0_cs=66), _EALIGN), (dict(f1_cs=66), _EALIGN),
    (dict(_BIG), _ERANGE),                                                              # one image past 2^31 bytes
    (dict(f0=None, f1=_MIS), _EINVAL), (dict(N=0, R=5), _EINVAL), (dict(R=5, f0_cs=28), _EUNSUP), (dict(f0_cs=28, f0=_MIS), _EINVAL),
    (dict(out_cs=80, f1_cs=66), _EINVAL), (dict(_BIG, f0=_MIS), _EALIGN), (dict(_BIG, N=0), _EINVAL), (dict(_BIG, R=5), _EUNSUP))] + [
    # search range 3: the two plain entry points take it (rows with a second fault), the others refuse it
    ("pwc_cost_volume_f32", dict(R=3, out_cs=48), _EINVAL), ("pwc_cost_volume_f32", dict(R=3, f0=_MIS), _EALIGN),
    ("pwc_cost_volume_f32", dict(_BIG, R=3), _ERANGE), ("pwc_cost_volume_f32", dict(R=1, out_cs=8), _EINVAL),
    ("pwc_warp_cost_volume_f32", dict(R=3, out_cs=48), _EINVAL), ("pwc_warp_cost_volume_f32", dict(R=3, flow=None), _EINVAL),
    ("pwc_warp_cost_volume_f32", dict(_BIG, R=3), _ERANGE),
    ("pwc_warp_cost_volume_f32", dict(flow=None), _EINVAL), ("pwc_warp_cost_volume_f32", dict(flow_cs=1), _EINVAL),
    ("pwc_warp_cost_volume_f32", dict(_BIG, flow=None), _EINVAL), ("pwc_warp_cost_volume_f32", dict(flow=None, f0=_MIS), _EALIGN),
    ("pwc_warp_cost_volume_f32", dict(_BIG, flow=_MIS2), _ERANGE)] + [
    (name, bad, code) for name in _CV_COPY for bad, code in (
        (dict(R=3), _EUNSUP), (dict(R=3, f0_cs=28), _EUNSUP if name not in _CV_CONCAT else _EINVAL),
        (dict(R=3, f0=_MIS), _EUNSUP if name not in _CV_CONCAT else _EALIGN),
        (dict(flow_cs=1), _EINVAL), (dict(copy_cs=28), _EINVAL), (dict(copy=_MIS), _EALIGN), (dict(copy_cs=66), _EALIGN),
        (dict(flow_cs=1, R=5), _EUNSUP), (dict(copy_cs=28, f0=_MIS), _EINVAL if name not in _CV_CONCAT else _EALIGN),
        (dict(_BIG, copy=_MIS), _EALIGN if name not in _CV_CONCAT else _ERANGE))] + [
    ("pwc_cost_volume_coarse_f32", dict(flow_cs=1, R=3), _EUNSUP), ("pwc_cost_volume_coarse_f32", dict(H=4096, W=4096, f1_cs=128), _ERANGE)] + [
    (name, bad, code) for name in _CV_CONCAT for bad, code in (
        (dict(out=_MIS), _EALIGN), (dict(out_cs=86), _EALIGN), (dict(flow=_MIS2), _EALIGN),     # what only the buffer-resource kernels need
        (dict(pad=1, out_cs=81), _EINVAL), (dict(pad=1, out_cs=82), _EINVAL), (dict(pad=2, out_cs=82), _EINVAL),      # out_pad_writable with out_cs < 84
        (dict(pad=1, out_cs=82, R=3), _EINVAL), (dict(flow_cs=1, R=3), _EINVAL), (dict(pad=1, out_cs=82, f0=_MIS), _EALIGN),
        (dict(C=48, f0_cs=64, f1_cs=64, copy_cs=64), _EUNSUP), (dict(C=48, f0_cs=64, f1_cs=64, copy_cs=64, out=_MIS), _EUNSUP),
        (dict(C=16), _EUNSUP), (dict(C=256, f0_cs=256, f1_cs=256, copy_cs=256), _EUNSUP), (dict(R=3, out=_MIS), _EUNSUP),
        (dict(_BIG, out=_MIS), _ERANGE), (dict(_BIG, flow=_MIS2), _ERANGE),
        # the range part of a failed eligibility is reported as such only for `out` and f0
        (dict(_CV_WIDE, f1_cs=128), _EALIGN), (dict(_CV_WIDE, copy_cs=128), _EALIGN), (dict(_CV_WIDE, flow_cs=128), _EALIGN),
        (dict(_CV_WIDE, f0_cs=128), _ERANGE), (dict(_CV_WIDE, out_cs=128), _ERANGE))] + [
    # the channel sets of the two families
    ("pwc_warp_cost_volume_concat_f32", dict(C=128, f0_cs=128, f1_cs=128, copy_cs=128), _EUNSUP),
    ("pwc_warp_cost_volume_concat_h2_f32", dict(C=128, f0_cs=128, f1_cs=128, copy_cs=128), _EUNSUP),
    ("pwc_warp_cost_volume_concat_blk_f32", dict(C=32), _EUNSUP),
    # out_pad_writable == 2 (the flow in channels 81, 82): the h2 entry point only, and only with a flow
    ("pwc_warp_cost_volume_concat_f32", dict(pad=2), _EUNSUP), ("pwc_warp_cost_volume_concat_blk_f32", dict(pad=2), _EUNSUP),
    ("pwc_warp_cost_volume_concat_f32", dict(pad=2, out=_MIS), _EUNSUP), ("pwc_warp_cost_volume_concat_blk_f32", dict(pad=2, out=_MIS), _EUNSUP),
    ("pwc_warp_cost_volume_concat_f32", dict(_BIG, pad=2), _EUNSUP), ("pwc_warp_cost_volume_concat_blk_f32", dict(_BIG, pad=2), _EUNSUP),
    ("pwc_warp_cost_volume_concat_f32", dict(pad=2, flow_cs=1), _EINVAL), ("pwc_warp_cost_volume_concat_blk_f32", dict(pad=2, flow_cs=1), _EINVAL),
    ("pwc_warp_cost_volume_concat_h2_f32", dict(pad=2, flow=None), _EINVAL), ("pwc_warp_cost_volume_concat_h2_f32", dict(pad=2, flow=None, out=_MIS), _EALIGN),
    ("pwc_warp_cost_volume_concat_h2_f32", dict(_BIG, pad=2, flow=None), _ERANGE), ("pwc_warp_cost_volume_concat_h2_f32", dict(pad=2, out=_MIS), _EALIGN),
    ("pwc_warp_cost_volume_concat_h2_f32", dict(pad=2, flow=None, R=3), _EUNSUP), ("pwc_warp_cost_volume_concat_h2_f32", dict(_BIG, pad=2), _ERANGE),
]


def test_correlation_entry_points_report_the_same_codes():
    """The argument checks of the correlation entry points (plain, fused-warp, coarse and the three warp + cost volume + concat
    forms) go through one shared checker; every family keeps the rules that are its own (out_pad_writable == 2, the channel sets,
    which code a failed eligibility reports).  This table pins which code each entry point returns for a bad call -- one fault at a
    time, then two at once (which one wins) -- as recorded from the library before the checks were shared.  Every row fails a
    check: nothing is launched, no GPU is needed."""
    L = _lib.lib()
    assert all(code != 0 for _, _, code in _CV_FAULTS)
    assert {name for name, _, _ in _CV_FAULTS} == set(_CV_CALLS)
    got = []
    for name, bad, code in _CV_FAULTS:
        names, own = _CV_CALLS[name]
        good = dict(_CV_GOOD, **own)
        assert set(bad) <= set(good), (name, bad)
        args = dict(good, **bad)
        rc = getattr(L, name)(*[args[k] for k in names.split()])
        if rc != code:
            got.append((name, bad, code, rc))
    assert not got, got


def test_lrelu_grad_refuses_before_any_launch():
    """pwc_lrelu_grad_f32: misaligned pointers, strides or channel counts are PWC_EALIGN, a channel stride below C, a null
    pointer or an empty size PWC_EINVAL -- before any launch."""
    L = _lib.lib()
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    call = lambda y=p, y_cs=8, dy=p, dy_cs=8, npix=6, C=8: L.pwc_lrelu_grad_f32(y, y_cs, dy, dy_cs, npix, C, 0.1, None)
    assert call(y=odd) == _EALIGN and call(dy=odd) == _EALIGN and call(C=6, y_cs=6, dy_cs=6) == _EALIGN
    assert call(y_cs=10) == _EALIGN and call(dy_cs=9) == _EALIGN
    assert call(y_cs=4) == _EINVAL and call(dy_cs=7) == _EINVAL and call(y=None) == _EINVAL and call(npix=0) == _EINVAL
    assert call(C=0) == _EINVAL


def test_round5_routing_rules_are_host_logic():
    """Which kernel takes which launch is decided by pure host functions of the library (no GPU needed): the small-launch conv
    (up to 1e8 multiply-adds and 4096 output pixels; stride-2 / thin layers beyond), the weights-stationary thin-input conv
    (16 input channels, 32 output channels, at least 256 tiles), the block correlation (alignment only: the pixel limit is the
    caller's), packed sizes, and argument validation before any launch."""
    L = _lib.lib()
    sk = L.pwc_conv3x3_sk_supported
    # BASELINE configs[1], batch 8: estimator levels 0-1, the extractor's last levels (both frames stacked: N = 16)
    assert sk(8, 7, 16, 288, 128, 1, 1) == 1 and sk(8, 14, 32, 128, 128, 1, 1) == 1 and sk(16, 14, 32, 128, 192, 2, 1) == 1
    assert sk(8, 14, 32, 256, 128, 1, 1) == 1            # patch in the LDS (stride 1, 96 ... 288 channels): up to 2.4e8 multiply-adds
    assert sk(16, 14, 32, 128, 128, 1, 1) == 1 and sk(8, 28, 64, 128, 128, 1, 1) == 0     # up to 8 K output pixels
    assert sk(8, 28, 64, 224, 128, 1, 1) == 0            # 4.1e8: conv3x3_h2_kernel is faster (measured)
    assert sk(8, 56, 128, 128, 96, 1, 1) == 0            # 57344 output pixels
    assert sk(16, 14, 32, 128, 128, 1, 2) == 0           # dilated: fragments from global memory, 7168 pixels, not thin
    assert sk(16, 28, 64, 96, 128, 2, 1) == 1            # stride 2 beyond 4096 pixels
    assert sk(16, 56, 128, 64, 96, 2, 1) == 1            # 1.76e8 multiply-adds at stride 2: against the fp32-pipe kernel (measured)
    assert sk(16, 112, 256, 32, 64, 2, 1) == 0
    assert sk(8, 28, 64, 64, 32, 1, 1) == 1              # thin layer beyond 4096 pixels
    assert sk(8, 112, 256, 128, 128, 1, 1) == 0 and sk(8, 7, 16, 48, 128, 1, 1) == 0 and sk(8, 7, 16, 64, 24, 1, 1) == 0
    assert sk(1, 112, 256, 32, 32, 1, 1) == 1            # a single pair: 28672 pixels but 2.9e7 multiply-adds
    assert L.pwc_conv3x3_sk_packed_floats(288, 128) == 9 * 288 * 128 and L.pwc_conv3x3_sk_packed_floats(48, 128) == 0
    t32 = L.pwc_conv3x3_t32_supported
    assert t32(16, 224, 512, 16, 32, 2) == 1 and t32(16, 112, 256, 32, 32, 1) == 0 and t32(16, 224, 512, 16, 16, 2) == 0
    assert t32(1, 64, 128, 16, 32, 2) == 0               # 16 tiles: not worth a persistent launch
    assert L.pwc_conv3x3_t32_packed_floats(16) == 9 * 512 and L.pwc_conv3x3_t32_packed_floats(32) == 18 * 512
    blk = L.pwc_warp_cost_volume_concat_blk_supported
    assert blk(7, 16, 192, 4, 192, 192, 0, 288, 288) == 1 and blk(14, 32, 128, 4, 128, 128, 2, 256, 256) == 1
    assert blk(14, 32, 32, 4, 32, 32, 2, 128, 0) == 0 and blk(14, 32, 128, 3, 128, 128, 2, 256, 256) == 0
    assert blk(14, 32, 128, 4, 130, 128, 2, 256, 256) == 0      # channel stride % 4
    assert L.pwc_conv3x3_h2_stride2_supported(16, 224, 512, 16, 32) in (0, 1)
    # validation before any launch
    assert L.pwc_conv3x3_sk_f32(None, 32, None, None, None, 32, 1, 4, 4, 32, 32, 1, 1, 1, 0.1, None) == -1
    assert L.pwc_conv3x3_t32_f32(None, 16, None, None, None, 32, 1, 4, 4, 16, 32, 1, 1, 0.1, None) == -1
    assert L.pwc_warp_cost_volume_concat_blk_f32(None, 128, None, 128, None, 0, 1.0, None, 84, 1, None, 0, 1, 4, 4, 128, 4, 0.1, None) == -1


def test_effective_streams_rule():
    """PWCDCNet.effective_streams: the one place that decides into how many sub-batches a batch is cut (bench.py asks the model
    instead of restating the rule).  Constructing the model needs the library, not a GPU... but its VariableStore allocates
    on the device, so the rule is exercised on the unbound method with a stand-in object."""
    import types
    from pwcnet_amd.model import PWCDCNet
    rule = PWCDCNet.effective_streams
    auto = types.SimpleNamespace(streams=None)
    assert rule(auto, (8, 448, 1024, 3)) == 1 and rule(auto, (4, 64, 128, 3)) == 1       # round 5: one stream (measured)
    assert rule(auto, (2, 448, 1024, 3)) == 1 and rule(auto, (2, 128, 192, 3)) == 1
    dc = types.SimpleNamespace(streams=None, use_dc=True)
    assert rule(dc, (8, 448, 1024, 3)) == 1
    assert rule(auto, (1, 448, 1024, 3)) == 1 and rule(auto, (3, 448, 1024, 3)) == 1 and rule(auto, (7, 448, 1024, 3)) == 1
    two, one, four = (types.SimpleNamespace(streams=k) for k in (2, 1, 4))
    assert rule(two, (6, 64, 64, 3)) == 2 and rule(two, (5, 64, 64, 3)) == 1 and rule(one, (8, 448, 1024, 3)) == 1
    assert rule(four, (8, 64, 64, 3)) == 4 and rule(four, (6, 64, 64, 3)) == 1 and rule(four, (2, 64, 64, 3)) == 1


def test_side_stream_probe_inconclusive_falls_back_to_one_stream(monkeypatch):
    """eight ranks of a node run the side-stream probe at the same time (one per GPU, sharing the host).  When the
    probe cannot tell -- the spin kernel did not spin, or every candidate looks as if it shared the caller's queue -- the decision
    must be "single stream" with a report that says why, never an un-vetted side stream and never an exception.  No GPU here: the
    streams, events and the probe kernels are stand-ins; eight threads run the decision concurrently."""
    import threading
    import types
    import torch
    from pwcnet_amd import model as M

    class FakeStream:
        n = 0
        lock = threading.Lock()

        def __init__(self, device=None):
            with FakeStream.lock:
                FakeStream.n += 1
                self.cuda_stream = 1000 + FakeStream.n
    fake_cuda = types.SimpleNamespace(Stream=FakeStream, synchronize=lambda *a, **k: None, is_current_stream_capturing=lambda: False)
    fake_torch = types.SimpleNamespace(cuda=fake_cuda, zeros=lambda n, device=None: torch.zeros(n))
    monkeypatch.setattr(M, "torch", fake_torch)
    verdicts = {"stuck": (True, 0.001, 0.001),        # the spin did not spin: no verdict possible
                "shared": (True, 1.0, 1.0)}           # every candidate finishes behind the spin: all share the caller's queue
    for kind, answer in verdicts.items():
        monkeypatch.setattr(M, "_shares_queue", lambda dev, a, b, probe, spin_ticks=0, _a=answer: _a)
        out = [None] * 8
        def run(i):
            out[i] = M._pick_side_streams("cuda:%d" % i, FakeStream(), 1)
        th = [threading.Thread(target=run, args=(i,)) for i in range(8)]
        [t.start() for t in th]
        [t.join() for t in th]
        for i, (picked, report) in enumerate(out):
            assert picked is None, (kind, i)
            assert report["verdict"] == "only 0 of 1 vetted: single stream" and report["picked"] == []
            assert report["rejected"] >= 8 and report["device"] == "cuda:%d" % i and len(report["probes"]) >= 8
    # ... and a clean probe picks the first candidate
    monkeypatch.setattr(M, "_shares_queue", lambda dev, a, b, probe, spin_ticks=0: (False, 1.0, 0.01))
    picked, report = M._pick_side_streams("cuda:0", FakeStream(), 1)
    assert picked is not None and len(picked) == 1 and report["verdict"] == "vetted"
    # the model then runs the batch on ONE stream: the forward with no vetted side stream returns None from the side-stream path
    net = types.SimpleNamespace(_side_streams={}, side_stream_report=None)
    monkeypatch.setattr(M, "_shares_queue", lambda dev, a, b, probe, spin_ticks=0: (True, 0.001, 0.001))
    streams, rep = M._pick_side_streams("cuda:0", FakeStream(), 1)
    assert streams is None and "single stream" in rep["verdict"]


def test_product_never_imports_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pwcnet_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("SURVEY", ""), f"{f} mentions the oracle"


def test_cpu_tensors_are_rejected_not_computed_elsewhere():
    import torch
    import pwcnet_amd
    with pytest.raises(_lib.PwcHipError):
        pwcnet_amd.WarpingLayer("bilinear")(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4, 4, 2))


# ------------------------------------------------------------------ inventory / layouts
def test_conv_specs_match_checkpoint_index(golden_dir):
    _, entries = ckpt.read_index(os.path.join(golden_dir, "model_600.ckpt.index"))
    assert len(entries) == 333
    mv = ckpt.model_variables(entries)
    specs = W.conv_specs()
    assert len(mv) == 2 * len(specs) == 110
    for name, cin, cout in specs:
        assert mv[name + "/kernel"].shape == (3, 3, cin, cout) and mv[name + "/kernel"].dtype == ckpt.DT_FLOAT
        assert mv[name + "/bias"].shape == (cout,)
    assert sum(int(np.prod(e.shape)) for e in mv.values()) == W.num_parameters(specs) == 5029868
    assert max(e.offset + e.size for e in entries.values()) == 60358428
    assert entries["Variable"].dtype == ckpt.DT_INT32 and entries["Variable"].shape == ()
    assert "pwcdcnet/optflow_5/conv2d/kernel" not in entries


def test_estimator_channel_counts():
    assert [W.estimator_in_channels(l, False) for l in range(5)] == [273, 243, 211, 179, 147]
    assert [W.estimator_in_channels(l, True) for l in range(5)] == [273, 932, 1559, 2154, 2717]
    assert [W.estimator_feature_channels(l, True) for l in range(5)] == [721, 1380, 2007, 2602, 3165]
    assert W.num_parameters(W.conv_specs(use_dc=True)) == 40182338


@pytest.mark.parametrize("use_dc", [False, True])
def test_layouts_are_aligned_bijective_and_zero_padded(use_dc):
    for l in range(5):
        lay = W.estimator_layout(l, use_dc)
        p2l = np.asarray(lay.phys2log)
        assert lay.n_phys % 16 == 0 and lay.n_logical == W.estimator_feature_channels(l, use_dc) if use_dc \
            else lay.n_logical == W.estimator_in_channels(l, use_dc)
        assert sorted(p2l[p2l >= 0].tolist()) == list(range(lay.n_logical))      # bijection onto logical
        for name, (off, ln) in lay.segments.items():
            assert off % 4 == 0
        if use_dc:
            # conv k reads the suffix that starts where conv k-1 wrote / where cv starts
            starts = [lay.offset("cv")] + [lay.offset(f"conv{k}") for k in range(5)]
            assert all(s % 16 == 0 for s in starts)
            done = 0
            for k in range(5):
                m = lay.cin_map(starts[k], logical_base=448 - done)
                cin = lay.n_logical - (448 - done)
                assert sorted(m[m >= 0].tolist()) == list(range(cin))
                done += W.FILTERS_OF[k]
    cx = W.context_layout(use_dc)
    assert cx.n_logical == (3167 if use_dc else 34) and cx.offset("features") == 4


def test_layout_reorders_like_tf_concat():
    lay = W.estimator_layout(2, False)                      # [cv81 | f0 96 | flow 2 | feat_up 32]
    p2l = np.asarray(lay.phys2log)
    assert list(p2l[:81]) == list(range(81)) and list(p2l[81:84]) == [-1] * 3
    off = lay.offset("f0")
    assert off == 84 and list(p2l[off:off + 96]) == list(range(81, 177))
    assert list(p2l[lay.offset("flow"):lay.offset("flow") + 4]) == [177, 178, -1, -1]
    assert list(p2l[lay.offset("feat_up"):lay.offset("feat_up") + 32]) == list(range(179, 211))


def test_glorot_init_is_seeded_and_bounded():
    specs = W.conv_specs()
    a, b = W.init_weights(specs, seed=0), W.init_weights(specs, seed=0)
    k = "pwcdcnet/optflow_4/conv2d/kernel"
    assert np.array_equal(a[k], b[k]) and a[k].shape == (3, 3, 147, 128)
    assert np.abs(a[k]).max() <= np.sqrt(6.0 / (9 * 147 + 9 * 128)) and not np.any(a["pwcdcnet/context/conv2d/bias"])
    assert not np.array_equal(a[k], W.init_weights(specs, seed=1)[k])


# ------------------------------------------------------------------ checkpoint bundle
def test_bundle_round_trip_and_crc(tmp_path):
    specs = W.conv_specs()[:4] + W.conv_specs()[-2:]
    w = W.randomize_biases(W.init_weights(specs, seed=3))
    prefix = str(tmp_path / "model_1.ckpt")
    ckpt.save_weights(prefix, w)
    back = ckpt.load_weights(prefix)
    assert set(back) == set(w)
    for k in w:
        np.testing.assert_array_equal(back[k], w[k])
    # corrupt one byte of the data file -> CRC failure
    with open(prefix + ".data-00000-of-00001", "r+b") as f:
        f.seek(100); b = f.read(1); f.seek(100); f.write(bytes([b[0] ^ 0xFF]))
    with pytest.raises(ValueError, match="CRC32C"):
        ckpt.load_weights(prefix)
    # corrupt the index -> block CRC failure
    raw = bytearray(open(prefix + ".index", "rb").read()); raw[10] ^= 0xFF
    open(prefix + ".index", "wb").write(bytes(raw))
    with pytest.raises(ValueError):
        ckpt.read_index(prefix + ".index")


def test_reference_index_without_data_blob_reports_missing(golden_dir):
    with pytest.raises(FileNotFoundError, match="data-00000-of-00001"):
        ckpt.load_weights(os.path.join(golden_dir, "model_600.ckpt"))
    assert ckpt.crc32c(b"123456789") == 0xE3069283          # CRC-32C check value


def test_load_weights_strict_rejects_wrong_variable_sets():
    """tf.train.Saver.restore raises on a missing / mis-shaped tensor; so does load_weights
    (checked before anything is copied to a device, so this runs without a GPU)."""
    import pwcnet_amd
    from pwcnet_amd import weights as W
    w = W.init_weights(W.conv_specs())
    net = pwcnet_amd.PWCDCNet()
    with pytest.raises(ValueError, match="missing"):
        net.load_weights({})
    with pytest.raises(ValueError, match="missing"):
        net.load_weights({k.replace("pwcdcnet/", "other/"): v for k, v in w.items()})
    with pytest.raises(ValueError):
        pwcnet_amd.PWCDCNet(use_dc=True).load_weights(w)
    bad = dict(w)
    bad["pwcdcnet/context/conv2d/bias"] = np.zeros((64,), np.float32)
    with pytest.raises(ValueError, match="shape"):
        net.load_weights(bad)


def test_forward_pipeline_host_side():
    """pwcnet_amd.ForwardPipeline (round 6) without a GPU: `depth` replicas of PWCDCNet that keep their status copy in line,
    the model's kwargs passed through, the pipeline's own business (`streams`, `persistent_outputs`) refused, load_weights
    fanned out with the model's strictness, nothing of the oracle imported."""
    import pwcnet_amd
    from pwcnet_amd import pipeline
    pipe = pwcnet_amd.ForwardPipeline(depth=3, device="cuda:0", use_dc=True, output_level=3)
    assert len(pipe.nets) == 3 and pipe.depth == 3 and pipe.effective_depth == 0
    assert all(n.use_dc and n.output_level == 3 and n.streams == 1 and n.status_copy_on_caller_stream for n in pipe.nets)
    assert pwcnet_amd.PWCDCNet().status_copy_on_caller_stream is False
    assert len({id(n.store) for n in pipe.nets}) == 3            # replicas share no state
    for bad in ({"streams": 2}, {"persistent_outputs": True}):
        with pytest.raises(AssertionError):
            pwcnet_amd.ForwardPipeline(depth=2, device="cuda:0", **bad)
    with pytest.raises(ValueError, match="missing"):
        pipe.load_weights({})
    import torch
    with pytest.raises(ValueError, match="CUDA tensors"):      # (CPU tensors are refused like PWCDCNet refuses them: no fallback path)
        pipe.submit(torch.zeros((1, 64, 64, 3)), torch.zeros((1, 64, 64, 3)))
    src = open(pipeline.__file__).read()
    assert "oracle" not in src and "subprocess" not in src


# ------------------------------------------------------------------ sharding
def test_shard_range_partitions():
    for n, world in [(64, 8), (8, 8), (10, 4), (3, 8), (0, 2)]:
        parts = [sharding.shard_range(n, world, r) for r in range(world)]
        assert parts[0][0] == 0 and parts[-1][1] == n
        assert all(parts[i][1] == parts[i + 1][0] for i in range(world - 1))
        sizes = [b - a for a, b in parts]
        assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        sharding.shard_range(8, 2, 2)
    assert sharding.gather_stats({"pairs": 8.0, "seconds": 1.5}) == [{"pairs": 8.0, "seconds": 1.5}]


_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from pwcnet_amd import sharding
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
lo, hi = sharding.shard_range(10, w, r)
stats = sharding.gather_stats({"pairs": float(hi - lo), "seconds": 1.0 + r, "lo": float(lo)}, dist, "cpu")
assert len(stats) == w and [s["seconds"] for s in stats] == [1.0 + i for i in range(w)]
assert sum(s["pairs"] for s in stats) == 10 and stats[r]["lo"] == lo
if r == 0:
    print("GATHER_OK", max(s["seconds"] for s in stats), sum(s["pairs"] for s in stats))
dist.destroy_process_group()
"""


def test_gather_stats_world2_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29617", str(script), ROOT],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "GATHER_OK 2.0 10.0" in out.stdout


_WORLD8_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from pwcnet_amd import sharding
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
steps, per_gpu_batch = 20, 8
# what bench.py hands to the gather on every rank: its pairs and ITS elapsed seconds (rank 5 is the slowest)
mine = {"pairs": float(per_gpu_batch * steps), "seconds": 0.070 + 0.001 * r + (0.010 if r == 5 else 0.0),
        "issue_seconds": 0.010 + 0.001 * r}
stats = sharding.gather_stats(mine, dist, "cpu")
# (bench.py prints every rank's ms per step beside the job's: the straggler is rank 5, visibly)
per_rank_ms = [1e3 * st["seconds"] / steps for st in stats]
assert len(per_rank_ms) == 8 and max(range(8), key=lambda i: per_rank_ms[i]) == 5
value, ms_per_step, total, n = sharding.aggregate_throughput(stats, steps)
assert n == w == 8 and total == 8 * per_gpu_batch * steps
slowest = 0.070 + 0.005 + 0.010
assert abs(ms_per_step - 1e3 * slowest / steps) < 1e-9 and abs(value - total / slowest) < 1e-6
# every rank computes the same aggregate (the gather is an ALL-gather)
agg = sharding.gather_stats({"value": value}, dist, "cpu")
assert all(abs(a["value"] - value) < 1e-9 for a in agg)
if r == 0:
    print("WORLD8_OK", n, int(total), round(value, 3))
dist.destroy_process_group()
"""


def test_bench_aggregation_world8_gloo(tmp_path):
    """The host logic of the 8-GPU bench line (BASELINE configs[2]) on 8 gloo ranks: value = sum of the ranks' pairs /
    the SLOWEST rank's seconds, ms_per_step from that rank, n_gpus = world -- so that the first real 8-GPU run cannot
    trip on the aggregation."""
    script = tmp_path / "world8_worker.py"
    script.write_text(_WORLD8_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
                          "--master-addr", "127.0.0.1", "--master-port", "29621", str(script), ROOT],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "WORLD8_OK 8 1280 15058.824" in out.stdout


def test_bench_config_presets_imply_their_gpu_count():
    """`--config configs2` / `configs4` are BASELINE's 8- and 2-GPU configurations; an explicit --gpus wins."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--config", "configs4"])
    assert (a.gpus, a.height, a.width, a.batch, a.gpus_given) == (2, 960, 1920, 8, False)
    assert bench.parse(["--config", "configs2"]).gpus == 8
    a = bench.parse(["--config", "configs4", "--gpus", "1"])
    assert a.gpus == 1 and a.gpus_given
    assert bench.parse(["--config", "configs3"]).gpus == 1 and bench.parse(["--config", "configs3"]).use_dc


def test_bench_dump_outputs_caps_its_bytes_with_a_fixed_sample(tmp_path):
    """bench.dump_outputs: float32 .npy files, whole arrays under the budget; over it, every array becomes the same seeded
    sample of its share on every call.  A plain run is the headline only (--full off by default)."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None and bench.parse(["--full", "--dump-outputs", "x"]).full
    big = np.arange(1000, dtype=np.float64).reshape(10, 100)
    small = np.ones((3, 4), np.float32)
    w = bench.dump_outputs(str(tmp_path / "whole"), {"big": big, "small": small})
    assert w == {"big.npy": (10, 100), "small.npy": (3, 4)}
    got = np.load(tmp_path / "whole" / "big.npy")
    assert got.dtype == np.float32 and np.array_equal(got, big)
    budget = 1000                                   # bytes: 4000 + 48 in, 247 + 2 floats out
    w = bench.dump_outputs(str(tmp_path / "s1"), {"big": big, "small": small}, budget=budget, prefix="rank1_")
    bench.dump_outputs(str(tmp_path / "s2"), {"big": big, "small": small}, budget=budget, prefix="rank1_")
    s1 = np.load(tmp_path / "s1" / "rank1_big.npy")
    assert sum(4 * n for (n,) in w.values()) <= budget and len(s1) > 200
    assert np.array_equal(s1, np.load(tmp_path / "s2" / "rank1_big.npy"))
    assert np.all(np.diff(s1) > 0) and set(s1) <= set(big.ravel())         # sorted distinct elements of the array


_EVAL_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from pwcnet_amd import sharding
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
N, h, wd = 7, 6, 10                        # 7 pairs over 2 ranks: 4 + 3
rs = np.random.RandomState(3)
im = rs.rand(N, 2, h, wd, 3).astype(np.float32)
gt = rs.normal(size=(N, h, wd, 2)).astype(np.float32)
def load_pair(i):
    return torch.from_numpy(im[i, 0]), torch.from_numpy(im[i, 1]), torch.from_numpy(gt[i])
def forward(a, b):                         # a stand-in "network": flow = channel differences
    return torch.stack([(a - b)[..., 0], (a + b)[..., 1]], dim=3)
res = sharding.evaluate_pairs(forward, load_pair, N, batch=3, dist=dist, device="cpu", gather=True)
pred = np.stack([im[:, 0, ..., 0] - im[:, 1, ..., 0], im[:, 0, ..., 1] + im[:, 1, ..., 1]], axis=3)
norms = np.sqrt(((gt - pred) ** 2).sum(axis=3))
assert abs(res["epe"] - norms.mean()) < 1e-6 and res["pairs"] == N
assert np.allclose(res["per_pair_epe"], norms.mean(axis=(1, 2)), atol=1e-6)
assert tuple(res["flows"].shape) == (N, h, wd, 2) and np.allclose(res["flows"].numpy(), pred, atol=1e-6)
assert abs(float(sharding.epe(torch.from_numpy(gt), torch.from_numpy(pred))) - norms.mean()) < 1e-6
if r == 0:
    print("EVAL_OK", w)
dist.destroy_process_group()
"""


def test_sharded_evaluation_world2_gloo(tmp_path):
    """pairs sharded 4 + 3 over two ranks, flows and EPE statistics gathered."""
    script = tmp_path / "eval_worker.py"
    script.write_text(_EVAL_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29618", str(script), ROOT],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "EVAL_OK 2" in out.stdout


_EMPTY_RANK_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch, torch.distributed as dist
from pwcnet_amd import sharding
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
N, h, wd = 1, 6, 10                        # ONE pair over 2 ranks: rank 1 holds nothing
rs = np.random.RandomState(5)
im = rs.rand(N, 2, h, wd, 3).astype(np.float32)
gt = rs.normal(size=(N, h, wd, 2)).astype(np.float32)
def load_pair(i):
    return torch.from_numpy(im[i, 0]), torch.from_numpy(im[i, 1]), torch.from_numpy(gt[i])
def forward(a, b):
    return torch.stack([(a - b)[..., 0], (a + b)[..., 1]], dim=3)
res = sharding.evaluate_pairs(forward, load_pair, N, batch=3, dist=dist, device="cpu", gather=True)
pred = np.stack([im[:, 0, ..., 0] - im[:, 1, ..., 0], im[:, 0, ..., 1] + im[:, 1, ..., 1]], axis=3)
assert tuple(res["flows"].shape) == (N, h, wd, 2) and np.allclose(res["flows"].numpy(), pred, atol=1e-6)
assert res["pairs"] == 1 and len(res["per_pair_epe"]) == 1
if r == 0:
    print("EMPTY_RANK_OK", w)
dist.destroy_process_group()
"""


def test_sharded_evaluation_with_an_empty_rank_gloo(tmp_path):
    """n_pairs < world: the rank without pairs must pad to the shape the other ranks hold."""
    script = tmp_path / "empty_worker.py"
    script.write_text(_EMPTY_RANK_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29619", str(script), ROOT],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "EMPTY_RANK_OK 2" in out.stdout


_ALLREDUCE_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from pwcnet_amd import sharding
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
flat = torch.arange(10, dtype=torch.float32) * (r + 1)       # rank 0: k, rank 1: 2k
world = sharding.allreduce_sum_(flat, dist)
assert world == 2 and torch.equal(flat, torch.arange(10, dtype=torch.float32) * 3)
assert sharding.allreduce_sum_(flat.clone(), None) == 1
if r == 0:
    print("ALLREDUCE_OK", w)
dist.destroy_process_group()
"""


def test_gradient_allreduce_world2_gloo(tmp_path):
    """the training step's one collective -- the flat gradient buffer summed over the ranks."""
    script = tmp_path / "allreduce_worker.py"
    script.write_text(_ALLREDUCE_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29620", str(script), ROOT],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ALLREDUCE_OK 2" in out.stdout


# ------------------------------------------------------------------ flow IO (f2)
def test_flo_round_trip_and_layout(tmp_path):
    from pwcnet_amd import flow_io
    flow = np.random.RandomState(0).normal(size=(5, 7, 2)).astype(np.float32)
    p = str(tmp_path / "a.flo")
    flow_io.write_flo(p, flow)
    raw = open(p, "rb").read()
    assert len(raw) == 12 + 5 * 7 * 2 * 4
    assert np.frombuffer(raw[:4], "<f4")[0] == np.float32(202021.25)
    assert tuple(np.frombuffer(raw[4:12], "<i4")) == (7, 5)             # width first, then height
    np.testing.assert_array_equal(flow_io.read_flo(p), flow)
    open(p, "wb").write(b"\x00" * 20)
    with pytest.raises(ValueError):
        flow_io.read_flo(p)


def test_flow_color_wheel_and_crop():
    from pwcnet_amd import flow_io
    wheel = flow_io.color_wheel()
    assert wheel.shape == (55, 3)
    assert tuple(wheel[0]) == (255, 0, 0) and tuple(wheel[15]) == (255, 255, 0) and tuple(wheel[21]) == (0, 255, 0)
    assert tuple(wheel[54]) == (255, 0, 255 - np.floor(255 * 5 / 6))
    img = flow_io.flow_to_color(np.zeros((4, 6, 2), np.float32))
    assert img.dtype == np.uint8 and img.shape == (4, 6, 3) and (img == 255).all()     # zero flow is white
    f = np.zeros((1, 2, 2), np.float32)
    f[0, 0] = (1, 0)
    f[0, 1] = (-1, 0)
    c = flow_io.flow_to_color(f)
    assert not np.array_equal(c[0, 0], c[0, 1])                                        # opposite directions differ
    assert flow_io.factor_crop(np.zeros((130, 200, 3))).shape == (128, 192, 3)


def test_stale_counter_evidence_is_refused(tmp_path):
    """bench.traffic_stale: no stamp, another source hash, or another launch count per forward -> a reason (the traffic is not
    printed); the tree's own stamp with the same launch count -> None.  And the committed profiles/pmc_traffic.json either
    matches the committed kernel sources or will be reported as stale -- never printed as this run's evidence."""
    import json, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    from pwcnet_amd.profiler import source_stamp
    now = source_stamp()
    assert len(now) == 16 and now == source_stamp()
    fam = {"launches_per_forward": 23.0}
    assert bench.traffic_stale(None, fam, 23.0) is not None
    assert "kernel sources" in bench.traffic_stale({"source_sha": "0" * 16}, fam, 23.0)
    assert "launches per forward" in bench.traffic_stale({"source_sha": now}, fam, 24.0)
    assert bench.traffic_stale({"source_sha": now}, fam, 23.0) is None
    t = json.load(open(os.path.join(root, "profiles", "pmc_traffic.json")))
    st = t.get("stamp")
    verdict = bench.traffic_stale(st, t["kernels"].get("conv3x3_h2_kernel"), None)
    assert verdict is None or isinstance(verdict, str)
    if st and st.get("source_sha") == now:
        assert verdict is None and "conv3x3_h2_kernel" in st["kernel_symbols"]

"""Pins the bits of the fp32-matrix-pipe convolutions: the three weight packers (conv3x3_mfma / wino / wino4), the F(2x2) and
F(4x4) Winograd kernels, the F(2x2) channel split with its reduce kernel, and the MFMA implicit GEMM with its tap split and
its halo form.

These kernels have no atomics and sum in a fixed order -- the 16-channel stages in sequence, the channel-split and tap-split
partials in index order -- so their bits are a contract: the comparison is exact equality with a recording, no tolerance.  The
recording (tests/golden/conv_fp32_bits.json.gz) is written by tests/golden/make_conv_fp32_bits_golden.py from a library known
to be right and only re-recorded on purpose (a deliberate change of arithmetic).  Inputs are rebuilt here from
numpy.random.RandomState with fixed seeds.  An output is compared as the SHA-256 of its whole destination buffer -- padding
channels, prefilled with a sentinel, included -- with the first 16 words kept beside it for diagnosis.  Every call goes
through the C ABI, so that tile, split, strides and the alignment of y are the test's to choose.

Which instantiation of conv3x3_wino_kernel a shape reaches (wino_geo, wino_bn and the persistent rule of wino_run,
conv3x3_wino.hip), hs x ws the (sub-lattice) image:
  1x17x19 32->48 d1      17 x 19: 16x16 blocks (GEO 0), Cout % 32 != 0: 16 couts (NT 1); 2 x 2 ragged blocks x 3 = 12 workgroups
  3x122x125 16->64 d1    GEO 0 (4x64 blocks cover 124 x 128 of 128 x 128: less than 5 % saved); 192 pixel blocks x 2 = 384: NT 2
  1x14x37 32->16 d2      7 x 19, d*d even and at most 8 rows: two sub-lattices per workgroup (GEO 1), NT 1
  12x14x250 16->64 d2    7 x 125: GEO 1; 12 x 2 x 8 pixel blocks x 2 = 384: NT 2
  1x12x120 32->48 d1     12 x 128 against 16 x 128: 4x64 blocks (GEO 2), NT 1
  16x12x250 16->64 d1    GEO 2; 16 x 4 x 3 pixel blocks x 2 = 384: NT 2
  5x238x250 16->16 d1    GEO 0 (240 x 256 either way); 1200 tiles of 16 couts, Cin <= 32, more than 1024: PERSIST on 512 workgroups
  18x60x250 32->16 d1    60 x 256 against 64 x 256: GEO 2; 18 x 4 x 15 = 1080 tiles: PERSIST
  1x40x50 32->32 d3      14 x 17 sub-lattices, d*d odd: GEO 0, 18 pixel blocks: NT 1
  1x17x19 32->48, y_cs 51   GEO 0, NT 1, scalar stores;  the same shape without activation
  1x14x32 112->32        channel split: GEO 0, NT 1, 7 stages dealt 3, 2, 2 (csplit 3) and 4, 3 (csplit 2)"""
import gzip
import hashlib
import json
import os
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_fp32_bits.json.gz")
SLOPE = 0.1
SENTINEL = -7.5


def _rs(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


def _gpu(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _p(t, floats=0):
    import ctypes
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def _digest(buf):
    """A whole destination buffer: SHA-256 of its bytes and the bits of its first 16 floats."""
    torch.cuda.synchronize()
    a = np.ascontiguousarray(buf.cpu().numpy()).reshape(-1)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "head": a[:16].view(np.uint32).tolist()}


def _check(rc, what):
    from pwcnet_amd import _lib
    _lib.check(rc, what)


_ENTRY = {"mfma": "pwc_conv3x3", "wino": "pwc_conv3x3_wino", "wino4": "pwc_conv3x3_wino4"}


def _pack(fam, w, cin_phys, cin_map=None):
    """The (3, 3, Cin, Cout) kernel w in family fam's packed form, the buffer prefilled with the sentinel."""
    from pwcnet_amd import _lib
    L = _lib.lib()
    cin, cout = w.shape[2], w.shape[3]
    packed = torch.full((getattr(L, _ENTRY[fam] + "_packed_floats")(cin_phys, cout),), SENTINEL, dtype=torch.float32, device="cuda")
    wd = _gpu(w)
    cm = None if cin_map is None else _gpu(cin_map, np.int32)
    _check(getattr(L, _ENTRY[fam] + "_pack_f32")(_p(wd), None if cm is None else _p(cm), cin, cin_phys, cout, _p(packed),
                                                _lib.current_stream()), f"{fam} pack")
    torch.cuda.synchronize()
    return packed


# ------------------------------------------------------------------ packers
PACK_SHAPES = {"cin40of48_cout24": (40, 48, 24, False), "cin24of32_map": (24, 32, 24, True), "cin16_cout16": (16, 16, 16, False)}


def _pack_case(fam, key):
    cin, cin_phys, cout, mapped = PACK_SHAPES[key]
    rs = _rs("pack", key)
    w = rs.uniform(-1, 1, (3, 3, cin, cout)).astype(np.float32)
    cin_map = None
    if mapped:                                       # a permutation of the logical channels, the padding (-1) in between
        cin_map = np.full(cin_phys, -1, np.int32)
        cin_map[rs.permutation(cin_phys)[:cin]] = rs.permutation(cin)
    return {"packed": _digest(_pack(fam, w, cin_phys, cin_map))}


# ------------------------------------------------------------------ convolutions
def _conv_inputs(key, N, H, W, cin, cout, x_pad=0):
    rs = _rs("conv", key, N, H, W, cin, cout)
    x = rs.uniform(-1, 1, (N, H, W, cin + x_pad)).astype(np.float32)
    w = (rs.uniform(-1, 1, (3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rs.uniform(-0.5, 0.5, (cout,)).astype(np.float32)
    return _gpu(x), w, _gpu(b)


def _dest(N, Ho, Wo, y_cs, y_off):
    """The destination, every float the sentinel: y_off floats in front of the first record (an unaligned y), one record's
    worth behind the last."""
    return torch.full((y_off + N * Ho * Wo * y_cs + y_cs,), SENTINEL, dtype=torch.float32, device="cuda")


def _wino_case(fam, N, H, W, cin, cout, dil=1, y_pad=0, y_off=0, x_pad=0, act=1, csplit=0):
    from pwcnet_amd import _lib
    L = _lib.lib()
    x, w, b = _conv_inputs(fam, N, H, W, cin, cout, x_pad)
    packed = _pack(fam, w, cin)
    y = _dest(N, H, W, cout + y_pad, y_off)
    head = (_p(x), cin + x_pad, _p(packed), _p(b), _p(y, y_off), cout + y_pad, N, H, W, cin, cout, dil, act, SLOPE)
    s = _lib.current_stream()
    if csplit:
        ws = torch.full((L.pwc_conv3x3_wino_split_workspace_floats(N, H, W, cout, csplit),), SENTINEL, dtype=torch.float32, device="cuda")
        _check(L.pwc_conv3x3_wino_split_f32(*head, csplit, _p(ws), ws.numel(), s), "wino split")
    else:
        _check(getattr(L, _ENTRY[fam] + "_f32")(*head, s), fam)
    return {"y": _digest(y)}


def _mfma_case(N, H, W, cin, cout, stride=1, dil=1, tile=-1, split=0, y_pad=0, y_off=0):
    from pwcnet_amd import _lib
    L = _lib.lib()
    x, w, b = _conv_inputs("mfma", N, H, W, cin, cout)
    packed = _pack("mfma", w, cin)
    Ho, Wo = -(-H // stride), -(-W // stride)
    y = _dest(N, Ho, Wo, cout + y_pad, y_off)
    ws = None
    if split > 1:
        ws = torch.full((L.pwc_conv3x3_workspace_floats(N * Ho * Wo, cout),), SENTINEL, dtype=torch.float32, device="cuda")
    _check(L.pwc_conv3x3_f32(_p(x), cin, _p(packed), _p(b), _p(y, y_off), cout + y_pad, N, H, W, cin, cout, stride, dil, 1, SLOPE,
                             tile, split, None if ws is None else _p(ws), 0 if ws is None else ws.numel(), _lib.current_stream()),
           "conv3x3 mfma")
    return {"y": _digest(y)}


_TILE_BN = [128, 96, 64, 32, 16, 128, 96, 64, 32, 16, 128, 96, 64, 32, 16]       # g_tiles of conv3x3_mfma.hip

CASES = {}
for _fam in _ENTRY:
    for _k in PACK_SHAPES:
        CASES[f"pack/{_fam}/{_k}"] = (_pack_case, (_fam, _k), {})
for _name, _shape, _kw in [
        ("geo0_nt1", (1, 17, 19, 32, 48), {}), ("geo0_nt2", (3, 122, 125, 16, 64), {}),
        ("geo1_nt1", (1, 14, 37, 32, 16), dict(dil=2)), ("geo1_nt2", (12, 14, 250, 16, 64), dict(dil=2)),
        ("geo2_nt1", (1, 12, 120, 32, 48), {}), ("geo2_nt2", (16, 12, 250, 16, 64), {}),
        ("persist_geo0", (5, 238, 250, 16, 16), {}), ("persist_geo2", (18, 60, 250, 32, 16), {}),
        ("dil3", (1, 40, 50, 32, 32), dict(dil=3)),
        ("scalar_stores", (1, 17, 19, 32, 48), dict(y_pad=3, x_pad=4)), ("no_act", (1, 17, 19, 32, 48), dict(act=0)),
        ("split3", (1, 14, 32, 112, 32), dict(csplit=3)), ("split2", (1, 14, 32, 112, 32), dict(csplit=2)),
        ("split3_unaligned_y", (1, 14, 32, 112, 32), dict(csplit=3, y_off=1))]:
    CASES[f"wino/{_name}"] = (_wino_case, ("wino", *_shape), _kw)
for _name, _shape, _kw in [("ragged", (1, 17, 35, 48, 32), {}), ("dil2", (1, 30, 60, 64, 48), dict(dil=2)),
                           ("cin256", (2, 16, 32, 256, 32), {})]:
    CASES[f"wino4/{_name}"] = (_wino_case, ("wino4", *_shape), _kw)
for _t, _bn in enumerate(_TILE_BN):
    for _cin in (48, 32):                            # KC 16: the register-staged kernel, KC 32: the LDS-DMA one
        CASES[f"mfma/tile{_t}_cin{_cin}"] = (_mfma_case, (1, 13, 21, _cin, _bn), dict(tile=_t))
CASES["mfma/stride2"] = (_mfma_case, (2, 13, 21, 48, 64), dict(stride=2, tile=12))
CASES["mfma/dil2"] = (_mfma_case, (1, 13, 21, 32, 64), dict(dil=2, tile=7))
CASES["mfma/scalar_stores"] = (_mfma_case, (1, 13, 21, 48, 32), dict(tile=13, y_pad=3))
CASES["mfma/split3"] = (_mfma_case, (1, 9, 5, 64, 64), dict(tile=12, split=3))
CASES["mfma/split9"] = (_mfma_case, (1, 9, 5, 64, 64), dict(tile=12, split=9))
CASES["mfma/split3_unaligned_y"] = (_mfma_case, (1, 9, 5, 64, 64), dict(tile=12, split=3, y_off=1))
CASES["mfma/halo16"] = (_mfma_case, (1, 250, 270, 16, 16), {})
CASES["mfma/halo32"] = (_mfma_case, (1, 250, 270, 32, 32), {})


def record(case):
    """What the library computes for a case, JSON-ready."""
    fn, args, kw = CASES[case]
    return json.loads(json.dumps(fn(*args, **kw)))


@pytest.fixture(scope="module")
def golden():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (torch.cuda.is_available() is False)")
    with gzip.open(FIXTURE, "rb") as f:
        return json.loads(f.read().decode())


def test_the_recording_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)


def test_the_mfma_cases_reach_the_kernels_they_name():
    from pwcnet_amd import _lib
    L = _lib.lib()
    assert L.pwc_conv3x3_uses_halo_kernel(250 * 270, 16, 16, 1, 1) == 1 and L.pwc_conv3x3_uses_halo_kernel(250 * 270, 32, 32, 1, 1) == 1
    bm, bn = _lib.ctypes.c_int(), _lib.ctypes.c_int()
    for t, want in enumerate(_TILE_BN):
        assert L.pwc_conv3x3_tile_shape(t, bm, bn) == 0 and bn.value == want


@pytest.mark.parametrize("case", list(CASES))
def test_conv_fp32_kernel_bits(golden, case):
    got, exp = record(case), golden[case]
    assert sorted(got) == sorted(exp), (sorted(got), sorted(exp))
    bad = {k: (got[k], exp[k]) for k in exp if got[k] != exp[k]}
    for k, (g, e) in bad.items():
        print(f"{case} {k}: got {g} recorded {e}")
    assert not bad, f"{case}: {sorted(bad)} differ from the recording"

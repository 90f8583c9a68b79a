"""A/B of the strided tile kernel (conv3x3_s2.hip) against another build of the library (the parent commit's libpwc_hip.so):
pwc_conv3x3_sk_variant_f32 tile 50 against that build's pwc_conv3x3_sk_f32, and pwc_conv3x3_h2_stride2_f32 of both builds.
usage (from the repository root): python scripts/exp_s2_tile_ab.py OTHER_LIBPWC_HIP_SO [OUT_JSON]"""
import ctypes, sys, os, json
import numpy as np, torch
sys.path.insert(0, os.getcwd())
from pwcnet_amd import _lib
L = _lib.lib()
P = ctypes.CDLL(os.path.abspath(sys.argv[1]))
for n, (res, args) in _lib.SIGNATURES.items():
    f = getattr(P, n); f.restype = res; f.argtypes = args
p = lambda t: ctypes.c_void_p(t.data_ptr())
def timeit(fn, reps=40):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / reps)
    return min(best), max(best)
out = []
def sk(N, H, W, cin, cout):
    x = torch.randn(N, H, W, cin, device="cuda"); k = torch.randn(3, 3, cin, cout, device="cuda") * 0.05; b = torch.randn(cout, device="cuda")
    y = torch.empty(N, (H + 1) // 2, (W + 1) // 2, cout, device="cuda"); y2 = torch.empty_like(y)
    pk = torch.empty(L.pwc_conv3x3_sk_packed_floats(cin, cout), device="cuda")
    assert L.pwc_conv3x3_sk_pack_f32(p(k), None, cin, cin, cout, p(pk), None) == 0
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    old = lambda: P.pwc_conv3x3_sk_f32(p(x), cin, p(pk), p(b), p(y), cout, N, H, W, cin, cout, 2, 1, 1, 0.1, s)
    new = lambda: L.pwc_conv3x3_sk_variant_f32(p(x), cin, p(pk), p(b), p(y2), cout, N, H, W, cin, cout, 2, 1, 1, 0.1, 50, s)
    assert old() == 0 and new() == 0
    to, tn = timeit(old), timeit(new)
    d = float((y - y2).abs().max())
    line = dict(entry="sk", shape=[N, H, W, cin, cout], tiles=N * (((H + 1) // 2 + 3) // 4) * (((W + 1) // 2 + 31) // 32), old_us=to, new_us=tn, maxdiff=d)
    print(json.dumps(line), flush=True); out.append(line)
def h2(N, H, W, cin, cout):
    x = torch.randn(N, H, W, cin, device="cuda"); k = torch.randn(3, 3, cin, cout, device="cuda") * 0.05; b = torch.randn(cout, device="cuda")
    y = torch.empty(N, H // 2, W // 2, cout, device="cuda"); y2 = torch.empty_like(y)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fns = []
    for lib, yy in ((P, y), (L, y2)):
        pk = torch.empty(lib.pwc_conv3x3_h2_stride2_packed_floats(cin, cout), device="cuda")
        assert lib.pwc_conv3x3_h2_stride2_pack_f32(p(k), None, cin, cin, cout, p(pk), None) == 0
        nws = lib.pwc_conv3x3_h2_stride2_workspace_floats(N, H, W, cin, cout)
        ws = torch.full((max(nws, 4),), -1, dtype=torch.int32, device="cuda")
        fns.append((lambda lib=lib, pk=pk, ws=ws, nws=nws, yy=yy: lib.pwc_conv3x3_h2_stride2_f32(p(x), cin, p(pk), p(b), p(yy), cout, N, H, W, cin, cout, 1, 0.1, p(ws) if nws else None, nws, None, s)))
    assert fns[0]() == 0 and fns[1]() == 0
    to, tn = timeit(fns[0]), timeit(fns[1])
    d = float((y - y2).abs().max())
    line = dict(entry="h2s2", shape=[N, H, W, cin, cout], tiles=N * ((H // 2 + 3) // 4) * ((W // 2 + 31) // 32), old_us=to, new_us=tn, maxdiff=d)
    print(json.dumps(line), flush=True); out.append(line)
for N in (16, 18, 64, 8, 2):
    sk(N, 56, 128, 64, 96)
for N in (16, 64):
    sk(N, 28, 64, 96, 128)
sk(16, 14, 32, 128, 128)
for N in (16, 18, 64, 2):
    h2(N, 112, 256, 32, 64)
h2(2, 16, 64, 32, 64)
if len(sys.argv) > 2:
    json.dump(out, open(sys.argv[2], "w"), indent=1)

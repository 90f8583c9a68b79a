"""CPU tests of flow composition: the float64 restatement tests/compose_ref.py against hand values and against torch.autograd on a
float64 torch statement of the same formula, chain_flows' slicing against a plain loop on the restatement, every refusal
pwcnet_amd.compose raises before it calls the library, the library's own argument checks (they return before any launch), the
workspace size, and infer_continuous.py's --chain flag."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from pwcnet_amd import compose as C  # the feature: without it nothing here can be collected
from tests import compose_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def test_restatement_against_hand_values():
    ab = np.zeros((1, 2, 3, 2), np.float32)
    bc = np.arange(12, dtype=np.float32).reshape(1, 2, 3, 2)           # bc[y, x] = (6 y + 2 x, 6 y + 2 x + 1)
    ab[0, 0, 0] = (0.5, 0.25)                                          # q = (0.5, 0.25): all four corners
    ab[0, 0, 1] = (1.0, 1.0)                                           # q = (2, 1): the last pixel, every corner clamps onto it
    ab[0, 0, 2] = (0.5, 0.0)                                           # q = (2.5, 0): out of frame
    ab[0, 1, 0] = (1e10, 1e10)                                         # unknown
    ab[0, 1, 1] = (-1.0, -1.0)                                         # q = (0, 0), weights 0: corners (0,0) (0,1) (1,0) (1,1)
    ab[0, 1, 2] = (0.0, 0.0)
    vbc = np.ones((1, 2, 3), np.uint8)
    out, valid, A, geo = R.compose(ab, bc)
    assert valid[0].tolist() == [[True, True, False], [False, True, True]]
    assert geo.reason[0].tolist() == [[R.VALID, R.VALID, R.OUT_OF_FRAME], [R.SENTINEL_F, R.VALID, R.VALID]]
    # 0.75 (0.5 * 0 + 0.5 * 2) + 0.25 (0.5 * 6 + 0.5 * 8) = 2.5, and + 1 for the second channel
    assert out[0, 0, 0].tolist() == [0.5 + 2.5, 0.25 + 3.5]
    assert out[0, 0, 1].tolist() == [1.0 + 10.0, 1.0 + 11.0]
    assert out[0, 1, 1].tolist() == [-1.0 + 0.0, -1.0 + 1.0]
    assert out[0, 1, 2].tolist() == [10.0, 11.0]
    assert out[0, 0, 2].tolist() == [1e10, 1e10] and out[0, 1, 0].tolist() == [1e10, 1e10]
    assert A[0, 0, 0].tolist() == [3.0, 3.75]
    # a zero-weight corner still decides: mask (1, 1) out, and the pixel that samples (0, 0) exactly is invalid
    vbc[0, 1, 1] = 0
    geo = R.Geometry(ab, bc, None, vbc)
    assert geo.reason[0, 1, 1] == R.MASKED_CORNER and geo.reason[0, 0, 0] == R.MASKED_CORNER
    bc2 = bc.copy()
    bc2[0, 0, 1, 1] = np.nan
    assert R.Geometry(ab, bc2).reason[0, 1, 1] == R.SENTINEL_CORNER
    vab = np.ones((1, 2, 3), np.uint8)
    vab[0, 1, 2] = 0
    assert R.Geometry(ab, bc, vab).reason[0, 1, 2] == R.OWN_MASK
    # gradient by hand at g = e_(0,0,0),k=0: dab = (1 + dS0/dqx, dS0/dqy) = (1 + 2, 6); dbc: the four weights
    g = np.zeros((1, 2, 3, 2), np.float32)
    g[0, 0, 0, 0] = 1.0
    g[0, 0, 2] = np.nan                                                # invalid: never read
    r = R.compose_grad(ab, bc, g)
    assert r["dab"][0, 0, 0].tolist() == [3.0, 6.0] and float(np.abs(r["dab"]).sum()) == 9.0
    assert r["dbc"][0, :, :2, 0].tolist() == [[0.375, 0.375], [0.125, 0.125]] and float(r["dbc"].sum()) == 1.0
    assert r["m"].tolist() == [1.0]
    assert r["K"][0].tolist() == [[2, 2, 0], [2, 2, 8]]               # (1,2): two pixels whose four clamped corners are all it


def _torch_statement(ab, bc, geo):
    """out of a composition as differentiable float64 torch, on the restatement's constants (floors, clamps, validity)."""
    N, H, W = geo.shape
    xs = torch.arange(W, dtype=torch.float64)[None, None, :]
    ys = torch.arange(H, dtype=torch.float64)[None, :, None]
    n = torch.from_numpy(np.ascontiguousarray(geo.n))
    x0, x1, y0, y1 = (torch.from_numpy(a) for a in (geo.x0, geo.x1, geo.y0, geo.y1))
    wx = (xs + ab[..., 0] - x0)[..., None]
    wy = (ys + ab[..., 1] - y0)[..., None]
    S = ((1 - wy) * ((1 - wx) * bc[n, y0, x0] + wx * bc[n, y0, x1]) + wy * ((1 - wx) * bc[n, y1, x0] + wx * bc[n, y1, x1]))
    return ab + S


@pytest.mark.parametrize("shape,integer", [((2, 5, 7), False), ((3, 9, 15), False), ((2, 1, 257), False), ((3, 9, 15), True)])
def test_restatement_gradients_equal_torch_autograd(shape, integer):
    N, H, W = shape
    ab, bc, vab, vbc, g = R.random_case(N, H, W, seed=4000 + 10 * H + W, integer=integer)
    for mode in R.MODES:
        ma, mb = R.masks_of(mode, vab, vbc)
        out, valid, _, geo = R.compose(ab, bc, ma, mb)
        ref = R.compose_grad(ab, bc, g, ma, mb)
        # the statement is evaluated on cleaned inputs (what the rule excludes replaced by 0): autograd would carry 0 * NaN
        a = torch.from_numpy(geo.f).requires_grad_(True)
        b = torch.from_numpy(geo.B).requires_grad_(True)
        got = _torch_statement(a, b, geo)
        v = torch.from_numpy(valid)
        assert float((got.detach() - torch.from_numpy(out))[v].abs().max()) <= 1e-13
        (got * torch.from_numpy(g.astype(np.float64)))[v].sum().backward()
        assert float((a.grad - torch.from_numpy(ref["dab"])).abs().max()) <= 1e-13 * float(ref["dab_mag"].max())
        assert float((b.grad - torch.from_numpy(ref["dbc"])).abs().max()) <= 1e-13 * max(float(np.abs(ref["dbc"]).max()), 1.0)
        assert bool((a.grad[~v] == 0).all())
        assert int(ref["K"].sum()) == 4 * int(valid.sum())


# ------------------------------------------------------------------ chain_flows: the slicing
def _restatement_compose(flows_ab, flows_bc, valid_ab=None, valid_bc=None):
    """compose_flows' interface on CPU tensors, computed by the restatement."""
    out, valid, _, _ = R.compose(flows_ab.numpy(), flows_bc.numpy(), None if valid_ab is None else valid_ab.numpy(),
                                 None if valid_bc is None else valid_bc.numpy())
    return torch.from_numpy(out.astype(np.float32)), torch.from_numpy(valid)


def test_chain_flows_slices_as_a_plain_loop(monkeypatch):
    monkeypatch.setattr(C, "compose_flows", _restatement_compose)
    T, H, W = 5, 9, 15
    ab, _, vab, _, _ = R.random_case(T, H, W, seed=77)
    flows, valids = torch.from_numpy(ab), torch.from_numpy(vab)
    for masks in (None, valids):
        for K in (1, 2, 3, 5):
            got, mask = C.chain_flows(flows, masks, span=K)
            assert tuple(got.shape) == (T - K + 1, H, W, 2) and tuple(mask.shape) == (T - K + 1, H, W) and mask.dtype == torch.bool
            for i in range(T - K + 1):
                want, want_mask = R.chain([ab[j:j + 1] for j in range(i, i + K)],
                                          None if masks is None else [vab[j:j + 1] for j in range(i, i + K)])
                if K == 1:
                    want_mask = R.known(ab[i:i + 1]) & (True if masks is None else vab[i:i + 1] != 0)
                assert np.array_equal(mask[i:i + 1].numpy(), want_mask), (K, i)
                assert np.array_equal(got[i:i + 1].numpy()[want_mask], want[want_mask]), (K, i)
                if K > 1:
                    assert bool((got[i][~mask[i]] == 1e10).all())
            # the list form is the left fold
            lst, lst_mask = C.chain_flows([flows[j:j + 1] for j in range(K)], None if masks is None else [masks[j:j + 1] for j in range(K)])
            assert torch.equal(lst.view(torch.int32), got[0:1].view(torch.int32)) and torch.equal(lst_mask, mask[0:1])    # (bits: K = 1 keeps its NaN)
    # a list may carry a mask for some flows only
    a, m = C.chain_flows([flows[0:1], flows[1:2], flows[2:3]], [None, valids[1:2], None])
    want, want_mask = R.chain([ab[0:1], ab[1:2], ab[2:3]], [None, vab[1:2], None])
    assert np.array_equal(m.numpy(), want_mask) and np.array_equal(a.numpy()[want_mask], want[want_mask])


# ------------------------------------------------------------------ pwcnet_amd.compose: refusals before any library call
def test_python_functions_refuse_bad_arguments_on_the_cpu():
    import pwcnet_amd as P
    a, b = torch.zeros((2, 5, 7, 2)), torch.zeros((2, 5, 7, 2))
    ok = torch.ones((2, 5, 7), dtype=torch.bool)
    with pytest.raises(TypeError, match="flows_ab"):
        P.compose_flows(a.double(), b)
    with pytest.raises(TypeError, match="flows_bc"):
        P.compose_flows(a, b.half())
    with pytest.raises(ValueError, match="flows_ab"):
        P.compose_flows(torch.zeros((2, 5, 7, 3)), b)
    with pytest.raises(ValueError, match="flows_ab: empty"):
        P.compose_flows(torch.zeros((2, 0, 7, 2)), torch.zeros((2, 0, 7, 2)))
    with pytest.raises(ValueError, match="flows_bc: expected"):
        P.compose_flows(a, torch.zeros((2, 5, 8, 2)))
    with pytest.raises(TypeError, match="valid_ab"):
        P.compose_flows(a, b, valid_ab=torch.zeros((2, 5, 7)))
    with pytest.raises(ValueError, match="valid_bc: expected shape"):
        P.compose_flows(a, b, valid_bc=torch.zeros((2, 7, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="valid_ab: the mask must be contiguous"):
        P.compose_flows(a, b, valid_ab=torch.zeros((2, 7, 5), dtype=torch.bool).transpose(1, 2))
    with pytest.raises(ValueError, match="flows_ab: the tensor is on cpu"):
        P.compose_flows(a, b, ok, ok)
    with pytest.raises(TypeError, match="g: expected"):
        P.compose_grad(a, b, torch.zeros((2, 5, 7, 2), dtype=torch.float64))
    with pytest.raises(ValueError, match="g: expected shape"):
        P.compose_grad(a, b, torch.zeros((1, 5, 7, 2)))
    with pytest.raises(ValueError, match="flows_ab: the tensor is on cpu"):
        P.compose_grad(a, b, torch.zeros((2, 5, 7, 2)))
    with pytest.raises(TypeError, match="flows: expected a non-empty list"):
        P.chain_flows(a)
    with pytest.raises(TypeError, match="flows: expected a non-empty list"):
        P.chain_flows([])
    with pytest.raises(ValueError, match="valids: expected None or a list of 2"):
        P.chain_flows([a, b], [ok])
    with pytest.raises(TypeError, match="span: expected an integer"):
        P.chain_flows(a, span=2.0)
    for span in (0, 3, -1):
        with pytest.raises(ValueError, match="span: expected 1 <= span <= 2"):
            P.chain_flows(a, span=span)
    with pytest.raises(TypeError, match="flows: expected a torch.float32"):
        P.chain_flows([a, b], span=2)
    with pytest.raises(TypeError, match="valids: expected a torch.bool"):
        P.chain_flows(a, [ok, ok], span=2)
    with pytest.raises(ValueError, match="valids: expected shape"):
        P.chain_flows(a, ok[:1], span=2)
    with pytest.raises(ValueError, match="flows_ab: the tensor is on cpu"):
        P.chain_flows(a, ok, span=2)
    with pytest.raises(ValueError, match="flows_ab: the tensor is on cpu"):
        P.chain_flows([a, b])


def test_library_refuses_before_any_launch():
    from pwcnet_amd import _lib
    L = _lib.lib()
    EINVAL, EALIGN, ERANGE = -1, -2, -3
    p, odd, half = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(4100)
    size = L.pwc_flow_compose_grad_workspace_bytes
    assert size(3, 5, 7) == 8 * (2 * 3 * 5 * 7 + 3)
    assert size(1, 1, 1) == 8 * 3 and size(8, 448, 1024) == 8 * (2 * 8 * 448 * 1024 + 8)
    assert size(65535, 1, 1) == 8 * 3 * 65535
    assert size(0, 5, 7) == 0 and size(1, 0, 7) == 0 and size(1, 5, -1) == 0
    assert size(65536, 1, 1) == 0 and size(1, 1 << 16, 1 << 15) == 0          # the sizes the entry point refuses
    assert size(1, 1, (1 << 31) - 1) == 0 and size(1, 1, (1 << 31) - 65536) == 0
    assert size(1, 1, (1 << 31) - 1 - 65536) == 8 * (2 * ((1 << 31) - 1 - 65536) + 1)      # the largest row it takes

    def fwd(ab=p, ab_cs=2, bc=p, bc_cs=2, N=2, H=5, W=7, out=p, out_cs=2, valid=p):
        return L.pwc_flow_compose_f32(ab, ab_cs, bc, bc_cs, None, None, N, H, W, out, out_cs, valid, None)

    def grad(ab=p, ab_cs=2, bc=p, bc_cs=2, N=2, H=5, W=7, g=p, g_cs=2, ws=p, ws_bytes=1 << 20, dab=p, dab_cs=2, dbc=p, dbc_cs=2):
        return L.pwc_flow_compose_grad_f32(ab, ab_cs, bc, bc_cs, None, None, N, H, W, g, g_cs, ws, ws_bytes, dab, dab_cs, dbc,
                                           dbc_cs, 0, None)

    shared = (dict(ab=None), dict(bc=None), dict(N=0), dict(H=0), dict(W=0), dict(N=-1), dict(ab_cs=1), dict(bc_cs=1), dict(bc_cs=0))
    for fn in (fwd, grad):
        for bad in shared:
            assert fn(**bad) == EINVAL, (fn.__name__, bad)
        assert fn(N=65536) == ERANGE
        assert fn(N=1, H=1 << 16, W=1 << 15) == ERANGE
        # a row whose last pixels the int pixel index of the validity count cannot step over (it advances by up to 65536 past them)
        assert fn(N=1, H=1, W=(1 << 31) - 1) == ERANGE and fn(N=1, H=1, W=(1 << 31) - 65536) == ERANGE
        assert fn(ab=odd) == EALIGN and fn(bc=odd) == EALIGN
    for bad in (dict(out=None), dict(valid=None), dict(out_cs=1)):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(out=odd) == EALIGN
    for bad in (dict(g=None), dict(dab=None), dict(dbc=None), dict(g_cs=1), dict(dab_cs=1), dict(dbc_cs=1), dict(ws=None),
                dict(ws_bytes=size(2, 5, 7) - 1), dict(ws_bytes=0)):
        assert grad(**bad) == EINVAL, bad
    assert grad(g=odd) == EALIGN and grad(dab=odd) == EALIGN and grad(dbc=odd) == EALIGN
    assert grad(ws=half) == EALIGN                                                 # off an 8-byte boundary
    assert grad(ws=half, ws_bytes=0) == EALIGN and grad(ws=None, N=65536) == ERANGE    # the order of the header


# ------------------------------------------------------------------ infer_continuous.py
def test_infer_continuous_parser_accepts_chain(monkeypatch, capsys):
    spec = importlib.util.spec_from_file_location("infer_continuous_under_test", os.path.join(ROOT, "infer_continuous.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    ap = cli.build_parser()
    assert ap.parse_args(["-i", "a.png", "b.png"]).chain == 0
    assert ap.parse_args(["-i", "a.png", "b.png", "c.png", "--chain", "2"]).chain == 2
    # K < 0 and K not below the number of frames are argument errors: exit status 2, before anything is loaded
    for chain in ("-1", "3", "7"):
        monkeypatch.setattr("sys.argv", ["infer_continuous.py", "-i", "a.png", "b.png", "c.png", "--chain", chain])
        with pytest.raises(SystemExit) as exit_info:
            cli.main()
        assert exit_info.value.code == 2 and "--chain must be" in capsys.readouterr().err
    assert "--chain K" in " ".join(cli.__doc__.split())
    assert cli.out_stem("seq/clip/frame_0001.png") == ["clip", "frame_0001"] and cli.out_stem("f.png") == ("", "f")

"""The three restatements of the forward agree at the degenerate geometries (CPU).

tests/test_oracle.py pins the C oracle (oracle/oracle.py), the numpy literal restatement (oracle/np_literal.py) and the float64
torch restatement (oracle/torch_ref.py) against one another at 64x128 only.  Before the float64 restatement is used as a
yardstick at frames 64 pixels wide or tall, these frames pin it there:

  (1, 64, 64)    levels 1x1 ... 16x16: the TF-legacy bilinear resize of 1x1 -> 2x2, stride-2 SAME on 2 -> 1 (pads bottom / right
                 only), a 9x9 search window larger than the map, the warp on a one-pixel map (border replication of a single
                 sample) and every dilation 2 ... 16 of the context network on a 16x16 map (at dilation 16, eight of nine taps
                 read padding);
  (1, 128, 64)   portrait: level widths 1, 2, 4, 8, 16 against heights 2 ... 32, the warp on a one-pixel-wide map;
  (1, 64, 192)   level heights 1 ... 16 against widths 3 ... 48: the resize of 1x3 -> 2x6.

Same inputs, gains and tolerances as test_torch_reference_forward_matches_the_oracle and
test_assembly_oracle_vs_literal_restatement."""
import numpy as np
import pytest
import torch

from oracle import np_literal as lit
from oracle import oracle as orc
from oracle import torch_ref as tr
from tests import util

FRAMES = [(1, 64, 64), (1, 128, 64), (1, 64, 192)]


def _inputs(shape, use_dc, gain):
    N, H, W = shape
    return util.model_weights(use_dc, gain=gain), util.smooth_images(N, H, W, seed=31, shift=(3, -2))


@pytest.mark.parametrize("use_dc", [False, True])
@pytest.mark.parametrize("shape", FRAMES)
def test_torch_reference_forward_matches_the_oracle_at(shape, use_dc):
    """C oracle (float32) against TorchPWCDCNet in float64."""
    N, H, W = shape
    w, (im0, im1) = _inputs(shape, use_dc, 1.2)
    o_final, o_pyr = orc.OraclePWCDCNet(w, use_dc=use_dc)(im0, im1)
    wt = {k: torch.tensor(v, dtype=torch.float64) for k, v in w.items()}
    with torch.no_grad():
        t_final, t_pyr = tr.TorchPWCDCNet(wt, use_dc=use_dc)(torch.tensor(im0, dtype=torch.float64),
                                                              torch.tensor(im1, dtype=torch.float64))
    assert float(np.abs(o_final).max()) > 0.5          # not a zero-flow triviality
    assert o_final.shape == tuple(t_final.shape) == (N, H, W, 2)
    assert [p.shape[1:3] for p in o_pyr] == [(H >> s, W >> s) for s in (6, 5, 4, 3, 2)]
    np.testing.assert_allclose(o_final, t_final.numpy(), rtol=0, atol=2e-4)
    assert len(o_pyr) == len(t_pyr) == 5
    for a, b in zip(o_pyr, t_pyr):
        assert a.shape == tuple(b.shape)
        np.testing.assert_allclose(a, b.numpy(), rtol=0, atol=1e-5)


@pytest.mark.parametrize("use_dc", [False, True])
@pytest.mark.parametrize("shape", FRAMES)
def test_assembly_oracle_vs_literal_restatement_at(shape, use_dc):
    """C oracle (float32) against the numpy literal restatement: flows and every level's features."""
    N, H, W = shape
    w, (im0, im1) = _inputs(shape, use_dc, 1.3 if not use_dc else 1.2)
    o_final, o_pyr, o_feats = orc.OraclePWCDCNet(w, use_dc=use_dc)(im0, im1, with_features=True)
    l_final, l_pyr, l_feats = lit.LiteralPWCDCNet(w, use_dc=use_dc)(im0, im1, with_features=True)
    assert float(np.abs(o_final).max()) > 0.5
    assert l_final.shape == o_final.shape == (N, H, W, 2)
    np.testing.assert_allclose(o_final, l_final, rtol=0, atol=2e-4)
    assert len(o_pyr) == len(l_pyr) == 5
    for a, b in zip(o_pyr, l_pyr):
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-5)
    assert len(o_feats) == len(l_feats)
    for a, b in zip(o_feats, l_feats):
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-5 * max(1.0, float(np.abs(b).max())))

"""CPU tests of the differentiable module's native entry point and constructor checks (no GPU: nothing is launched)."""
import ctypes
import os
import re

import pytest

from pwcnet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dgrad_s2_narrow_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "pwc_hip.h")).read()
    assert re.search(r"\bpwc_conv3x3_dgrad_s2_narrow_f32\s*\(", header)
    assert "pwc_conv3x3_dgrad_s2_narrow_f32" in _lib.SIGNATURES
    L = _lib.lib()
    f = L.pwc_conv3x3_dgrad_s2_narrow_f32
    assert f.argtypes == _lib.SIGNATURES["pwc_conv3x3_dgrad_s2_narrow_f32"][1]


def test_dgrad_s2_narrow_checks_its_arguments_before_any_launch():
    f = _lib.lib().pwc_conv3x3_dgrad_s2_narrow_f32
    al = ctypes.c_void_p(4096)      # (an aligned non-null address: argument checks only, nothing is launched)
    assert f(None, 16, al, al, 3, 1, 8, 8, 3, 16, 0, None) == -1           # null dy
    assert f(al, 16, None, al, 3, 1, 8, 8, 3, 16, 0, None) == -1           # null weights
    assert f(al, 16, al, None, 3, 1, 8, 8, 3, 16, 0, None) == -1           # null dx
    assert f(al, 16, al, al, 3, 0, 8, 8, 3, 16, 0, None) == -1             # empty batch
    assert f(al, 16, al, al, 3, 1, 7, 8, 3, 16, 0, None) == -4             # odd H
    assert f(al, 16, al, al, 3, 1, 8, 9, 3, 16, 0, None) == -4             # odd W
    assert f(al, 16, al, al, 5, 1, 8, 8, 5, 16, 0, None) == -4             # Cx above 4
    assert f(al, 16, al, al, 3, 1, 8, 8, 0, 16, 0, None) == -1             # Cx 0
    assert f(al, 16, al, al, 3, 1, 8, 8, 3, 18, 0, None) == -1             # dy_cs below Cy
    assert f(al, 20, al, al, 3, 1, 8, 8, 3, 18, 0, None) == -4             # Cy not a multiple of 4
    assert f(al, 16, al, al, 2, 1, 8, 8, 3, 16, 0, None) == -1             # dx_cs below Cx
    assert f(al, 18, al, al, 3, 1, 8, 8, 3, 16, 0, None) == -2             # dy_cs not a multiple of 4
    assert f(ctypes.c_void_p(4100), 16, al, al, 3, 1, 8, 8, 3, 16, 0, None) == -2   # dy not 16-byte aligned


@pytest.mark.parametrize("kw", [{"warp_type": "nearest"}, {"output_level": 3}, {"output_level": 2}, {"num_levels": 7}])
def test_module_refuses_unsupported_configurations(kw):
    from pwcnet_amd import PWCDCNetModule
    with pytest.raises(ValueError):
        PWCDCNetModule(**kw)

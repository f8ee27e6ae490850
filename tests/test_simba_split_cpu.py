"""The split SimBa plans' host side (include/agx_simba.h): the library's choice
inside the whole kernels' range, refusal of illegal plans before any HIP call,
and the workspace formula.  No device is needed."""

import ctypes
import os

import pytest

from agilerl_amd import _lib
from agilerl_amd.modules.simba import AgxSimbaDesc, AgxSimbaPlan


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def _desc(H, scale=4):
    d = AgxSimbaDesc()
    d.in_, d.H, d.scale, d.blocks, d.out_dim = 8, H, scale, 1, 8
    return d


@pytest.mark.parametrize("H,B", [(128, 64), (224, 256), (16, 5)])
def test_choice_inside_the_whole_kernels_range(lib, H, B):
    p = AgxSimbaPlan(9, 9, 9)
    assert lib.agx_simba_choose_plan(ctypes.byref(_desc(H)), B, ctypes.byref(p)) == 0
    assert (p.slices, p.row_tiles, p.w_parts) == (1, 1, 1)


@pytest.mark.parametrize("H,B,plan,word", [(128, 64, (17, 1, 1), b"slices"), (128, 64, (1, 3, 1), b"row tiles"),
                                           (128, 128, (1, 1, 5), b"row ranges"), (16, 64, (5, 1, 1), b"slices"),
                                           (512, 64, (1, 4, 1), b"LDS")])
def test_illegal_plans_are_refused_before_any_hip_call(lib, H, B, plan, word):
    d, p = _desc(H), AgxSimbaPlan(*plan)
    assert lib.agx_simba_forward_split(ctypes.byref(d), None, B, ctypes.byref(p), None, None) == -1
    assert word in lib.agx_last_error()
    assert lib.agx_simba_backward_split(ctypes.byref(d), None, B, None, None, ctypes.byref(p), None, None) == -1
    assert lib.agx_simba_split_workspace_bytes(ctypes.byref(d), B, ctypes.byref(p), 1) == 0


@pytest.mark.parametrize("H,scale,B,plan", [(496, 4, 64, (16, 2, 2)), (50, 2, 17, (1, 1, 2))])
def test_workspace_bytes_follow_the_header_formula(lib, H, scale, B, plan):
    S, _, Q = plan
    inner, nrt = scale * H, -(-B // 16)
    fwd = 1024 + 4 * (S * B * H if S > 1 else 0)
    bwd = fwd + 4 * (2 * B * H + 4 * nrt * H + (Q * (2 * inner * H + inner) if Q > 1 else 0))
    d, p = _desc(H, scale), AgxSimbaPlan(*plan)
    assert lib.agx_simba_split_workspace_bytes(ctypes.byref(d), B, ctypes.byref(p), 0) == fwd
    assert lib.agx_simba_split_workspace_bytes(ctypes.byref(d), B, ctypes.byref(p), 1) == bwd

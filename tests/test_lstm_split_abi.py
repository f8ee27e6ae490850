"""The split LSTM form's host side (include/agx_lstm.h): refusals before any HIP call, the workspace formula and
the chooser inside the whole kernels' range.  No device is needed."""

import ctypes
import os

import pytest

from agilerl_amd import _lib
from agilerl_amd.modules.lstm import AgxLstmDesc


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def _desc(H, L=1, n_in=8, pointers=True):
    d = AgxLstmDesc()
    d.in_, d.H, d.L = n_in, H, L
    if pointers:  # never dereferenced: every call below is refused before a launch
        for k in range(min(L, 4)):
            for name, _ in d.layer[k]._fields_:
                setattr(d.layer[k], name, 64)
    return d


@pytest.mark.parametrize("H,L,word", [(40, 1, b"multiple of 16"), (528, 1, b"multiple of 16"), (64, 5, b"layers")])
def test_bad_descriptors_are_refused(lib, H, L, word):
    d, p = _desc(H, L), ctypes.c_void_p(64)
    assert lib.agx_lstm_forward_split(ctypes.byref(d), p, p, p, 4, 2, p, p, p, None, p, None) == -1
    assert word in lib.agx_last_error()
    assert lib.agx_lstm_backward_split(ctypes.byref(d), p, p, p, 4, 2, p, p, p, None, None, None, None, None, p,
                                       None) == -1
    assert word in lib.agx_last_error()
    assert lib.agx_lstm_split_workspace_bytes(ctypes.byref(d), 4, 2, 1) == 0
    assert lib.agx_lstm_choose_plan(ctypes.byref(d), 4, 2, ctypes.byref(ctypes.c_int32())) == -1


def test_null_workspace_and_missing_parameters_are_refused(lib):
    p = ctypes.c_void_p(64)
    d = _desc(64)
    assert lib.agx_lstm_forward_split(ctypes.byref(d), p, p, p, 4, 2, p, p, p, None, None, None) == -1
    assert b"workspace" in lib.agx_last_error()
    assert lib.agx_lstm_backward_split(ctypes.byref(d), p, p, p, 4, 2, p, p, p, None, None, None, None, None, None,
                                       None) == -1
    assert b"workspace" in lib.agx_last_error()
    bare = _desc(64, pointers=False)
    assert lib.agx_lstm_forward_split(ctypes.byref(bare), p, p, p, 4, 2, p, p, p, None, p, None) == -1
    assert b"parameter is NULL" in lib.agx_last_error()


@pytest.mark.parametrize("H,L,B,T", [(144, 1, 130, 3), (512, 3, 7, 64), (16, 2, 1, 1)])
def test_workspace_bytes_follow_the_header_formula(lib, H, L, B, T):
    d, N = _desc(H, L, pointers=False), B * T
    assert lib.agx_lstm_split_workspace_bytes(ctypes.byref(d), B, T, 0) == 16 * N * H
    assert lib.agx_lstm_split_workspace_bytes(ctypes.byref(d), B, T, 1) == 4 * (N * H * (5 if L > 1 else 4) + B * H)


@pytest.mark.parametrize("H", [16, 64, 128])
@pytest.mark.parametrize("B,T", [(1, 1), (128, 64), (4096, 16)])
def test_the_chooser_keeps_narrow_layers_whole(lib, H, B, T):
    split = ctypes.c_int32(9)
    assert lib.agx_lstm_choose_plan(ctypes.byref(_desc(H, 2, pointers=False)), B, T, ctypes.byref(split)) == 0
    assert split.value == 0

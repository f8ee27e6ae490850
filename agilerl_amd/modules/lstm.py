"""Drop-in ``EvolvableLSTM`` (agilerl/modules/lstm.py) with the ``nn.LSTM``'s
forward and backward on agx_lstm_forward / _backward (include/agx_lstm.h,
csrc/lstm.hip).

Same constructor, attributes, module names (``{name}_lstm``, an ``nn.LSTM``
with ``batch_first``; ``{name}_lstm_output``, an ``nn.Linear``;
``{name}_output_activation``) and construction order, so a seeded build has
the reference's weights bit for bit and state dicts interchange.  The
parameters stay the ``nn.LSTM``'s own tensors.

``lstm_sequence(module, x, h0, c0)`` runs the stack on the fused kernels: x
[B, T, in], h0 / c0 [L, B, H] -> (y [B, T, H], h_n, c_n), one launch forward
(no-grad: nothing stored but the outputs) and three per layer backward.  That
is the ``"whole"`` plan; ``plan="split"`` runs the same arithmetic as one
launch per time step with every layer split by hidden unit across the device
(csrc/lstm_split.hip: agx_lstm_forward_split / _backward_split), bit for bit
the same results.  ``plan=None`` takes AGX_LSTM_PLAN=whole|split if set, else
agx_lstm_choose_plan's measured choice (split for wide layers).  It
applies to contiguous f32 CUDA tensors, 1..4 layers, H a multiple of 16 in
[16, 512], input sizes 1..512, zero inter-layer dropout or eval mode, modules
without hooks; anything else returns None and the torch module runs.  A
sequence run in chunks with the state carried has the bits of the sequence
run whole (step mode against the learner's sequence mode).

``EvolvableLSTM.forward`` takes the fused path under AGX_LSTM=1 wherever it
applies and never under AGX_LSTM=0.  Unset, it takes it in the cells where
tools/lstm_time.py measured it clear of torch (``_AUTO``).  That table
(profiles/lstm_time.json) could only time torch in eager calls,
so no bound is taken from it yet and every shape stays with torch."""

from __future__ import annotations

import copy
import ctypes
import os
from typing import Any

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _lib
from ._hooks import hooked
from .mlp import get_activation, preserve_parameters

_MAX_LAYERS, _MAX_HIDDEN, _MAX_INPUT, _MAX_ROWS = 4, 512, 512, 1 << 24
_LAYER_IN = ("w_ih", "w_hh", "b_ih", "b_hh")
# forward()'s own bounds: (max H, max layers) up to which the fused ranges lie clear of torch's in every measured
# cell of (mode, B, T); None: no like-for-like measurement yet, torch everywhere unless AGX_LSTM=1
_AUTO: tuple[int, int] | None = None


class AgxLstmLayer(ctypes.Structure):
    """Mirror of ``agx_lstm_layer`` (include/agx_lstm.h)."""

    _fields_ = [(n, ctypes.c_void_p) for n in _LAYER_IN] + [("g_" + n, ctypes.c_void_p) for n in _LAYER_IN]


class AgxLstmDesc(ctypes.Structure):
    """Mirror of ``agx_lstm_desc`` (include/agx_lstm.h)."""

    _fields_ = [("layer", AgxLstmLayer * _MAX_LAYERS)] + [(n, ctypes.c_int32) for n in ("in_", "H", "L")]


class EvolvableLSTM(nn.Module):
    LAYER_METHODS = ("add_layer", "remove_layer")
    NODE_METHODS = ("add_node", "remove_node")

    def __init__(self, input_size: int, hidden_state_size: int, num_outputs: int, num_layers: int = 1,
                 output_activation: str | None = None, min_hidden_state_size: int = 32,
                 max_hidden_state_size: int = 512, min_layers: int = 1, max_layers: int = 3, dropout: float = 0.0,
                 device="cpu", name: str = "lstm", random_seed: int | None = None) -> None:
        super().__init__()
        assert input_size > 0, "'input_size' cannot be less than or equal to zero, please enter a valid integer."
        assert hidden_state_size > 0, \
            "'hidden_state_size' cannot be less than or equal to zero, please enter a valid integer."
        assert num_outputs > 0, "'num_outputs' cannot be less than or equal to zero, please enter a valid integer."
        assert num_layers > 0, "'num_layers' cannot be less than or equal to zero, please enter a valid integer."
        assert min_hidden_state_size < max_hidden_state_size, \
            "'min_hidden_state_size' must be less than 'max_hidden_state_size'."
        assert min_layers < max_layers, "'min_layers' must be less than 'max_layers'."
        assert 0 <= dropout < 1, "'dropout' must be between 0 and 1."
        self.device, self.random_seed, self.name = device, random_seed, name
        self.rng = np.random.default_rng(seed=random_seed)
        self.input_size, self.hidden_state_size = input_size, hidden_state_size
        self.num_outputs, self.num_layers = num_outputs, num_layers
        self.output_activation = output_activation
        self.min_hidden_state_size, self.max_hidden_state_size = min_hidden_state_size, max_hidden_state_size
        self.min_layers, self.max_layers = min_layers, max_layers
        self.dropout = dropout
        self.last_mutation_attr: str | None = None
        self.disabled: set[str] = set()
        self.model = self.create_lstm()

    @property
    def hidden_state_architecture(self) -> dict[str, tuple[int, ...]]:
        """(layers, batch, hidden) of ``h`` and ``c`` (the states ``{name}_h`` / ``{name}_c``); the batch axis
        is -1 (the reference's BatchDimension)."""
        return {"h": (self.num_layers, -1, self.hidden_state_size),
                "c": (self.num_layers, -1, self.hidden_state_size)}

    def create_lstm(self) -> nn.ModuleDict:
        model = nn.ModuleDict()
        model[f"{self.name}_lstm"] = nn.LSTM(input_size=self.input_size, hidden_size=int(self.hidden_state_size),
                                             num_layers=self.num_layers, batch_first=True,
                                             dropout=self.dropout if self.num_layers > 1 else 0, device=self.device)
        model[f"{self.name}_lstm_output"] = nn.Linear(int(self.hidden_state_size), self.num_outputs,
                                                      device=self.device)
        model[f"{self.name}_output_activation"] = get_activation(self.output_activation)
        return model

    @property
    def net_config(self) -> dict[str, Any]:
        """Constructor arguments minus input_size / num_outputs / device / name (lstm.py:134-142)."""
        return dict(hidden_state_size=self.hidden_state_size, num_layers=self.num_layers,
                    output_activation=self.output_activation, min_hidden_state_size=self.min_hidden_state_size,
                    max_hidden_state_size=self.max_hidden_state_size, min_layers=self.min_layers,
                    max_layers=self.max_layers, dropout=self.dropout, random_seed=self.random_seed)

    @property
    def activation(self) -> None:
        return None

    @property
    def lstm(self) -> nn.LSTM:
        return self.model[f"{self.name}_lstm"]

    def lstm_output(self, x, hidden_state: dict[str, torch.Tensor] | None = None):
        """The ``nn.LSTM``'s half of ``forward``: -> (the top layer's output, [rows, H] for 2-D input, h_n, c_n)."""
        if not isinstance(x, torch.Tensor):
            x = torch.tensor(np.asarray(x), dtype=torch.float32, device=self.device)
        x_shape = x.shape
        if x.dim() == 2:
            x = x.unsqueeze(1)
        elif x.dim() != 3:
            raise ValueError("Expected 2D (batch_size, features) or 3D (batch_size, seq_len, features) input, "
                             f"but got {x.dim()}D")
        if hidden_state is None:
            raise ValueError("Hidden state is required for LSTM forward pass.")
        h0, c0 = hidden_state.get(f"{self.name}_h"), hidden_state.get(f"{self.name}_c")
        sequence_input = h0.shape[1] != x_shape[0]
        if sequence_input:  # [B * T, in] rows of B sequences
            x = x.view(h0.shape[1], -1, x_shape[1])
        fused = lstm_sequence(self, x, h0, c0) if _faster(self) else None
        out, (h_n, c_n) = (fused[0], fused[1:]) if fused is not None else self.lstm(x, (h0, c0))
        out = out.reshape(out.shape[0] * out.shape[1], out.shape[2]) if sequence_input else out.squeeze(1)
        return out, h_n, c_n

    def forward(self, x, hidden_state: dict[str, torch.Tensor] | None = None):
        out, h_n, c_n = self.lstm_output(x, hidden_state)
        out = self.model[f"{self.name}_lstm_output"](out)
        out = self.model[f"{self.name}_output_activation"](out)
        return out, {**hidden_state, f"{self.name}_h": h_n, f"{self.name}_c": c_n}

    def get_output_dense(self) -> nn.Module:
        return self.model[f"{self.name}_lstm_output"]

    def disable_mutations(self, kind: str | None = None) -> None:
        if kind in (None, "layer"):
            self.disabled.update(self.LAYER_METHODS)
        if kind in (None, "node"):
            self.disabled.update(self.NODE_METHODS)

    def change_activation(self, activation: str, output: bool = False) -> None:
        """Sets the output activation (lstm.py:153-163)."""
        self.output_activation = activation
        self.recreate_network()

    # ---- architecture mutations (lstm.py:238-296) ---------------------------
    def add_layer(self) -> dict[str, int] | None:
        self.last_mutation_attr = "add_layer"
        if self.num_layers < self.max_layers:
            self.num_layers += 1
            self.recreate_network()
            return None
        return self.add_node()

    def remove_layer(self) -> dict[str, int] | None:
        self.last_mutation_attr = "remove_layer"
        if self.num_layers > self.min_layers:
            self.num_layers -= 1
            self.recreate_network()
            return None
        return self.add_node()

    def add_node(self, numb_new_nodes: int | None = None) -> dict[str, int]:
        self.last_mutation_attr = "add_node"
        if numb_new_nodes is None:
            numb_new_nodes = int(self.rng.choice([16, 32, 64]))
        if self.hidden_state_size + numb_new_nodes <= self.max_hidden_state_size:
            self.hidden_state_size += numb_new_nodes
        self.recreate_network()
        return {"numb_new_nodes": numb_new_nodes}

    def remove_node(self, numb_new_nodes: int | None = None) -> dict[str, int]:
        self.last_mutation_attr = "remove_node"
        if numb_new_nodes is None:
            numb_new_nodes = int(self.rng.choice([16, 32, 64]))
        if self.hidden_state_size - numb_new_nodes >= self.min_hidden_state_size:
            self.hidden_state_size -= numb_new_nodes
        self.recreate_network()
        return {"numb_new_nodes": numb_new_nodes}

    def recreate_network(self) -> None:
        self.model = preserve_parameters(self.model, self.create_lstm())

    def clone(self) -> "EvolvableLSTM":
        return copy.deepcopy(self)


# ---- the fused path ---------------------------------------------------------
def enabled() -> bool:
    return os.environ.get("AGX_LSTM", "1") != "0"


def _faster(module: EvolvableLSTM) -> bool:
    """The shapes at which the fused path was measured faster, unless AGX_LSTM=1 asks for it everywhere."""
    if os.environ.get("AGX_LSTM") == "1":
        return True
    return _AUTO is not None and module.hidden_state_size <= _AUTO[0] and module.num_layers <= _AUTO[1]


def _plan(lstm: nn.LSTM):
    """((in, H, L), parameter tensors in descriptor order) of an nn.LSTM the kernels take, or None."""
    if (type(lstm) is not nn.LSTM or not lstm.batch_first or lstm.bidirectional or lstm.proj_size != 0 or
            not lstm.bias or not 1 <= lstm.num_layers <= _MAX_LAYERS or (lstm.dropout > 0 and lstm.training)):
        return None
    H, n_in = lstm.hidden_size, lstm.input_size
    if H % 16 or not 16 <= H <= _MAX_HIDDEN or not 1 <= n_in <= _MAX_INPUT:
        return None
    ts = [getattr(lstm, f"{n}_l{k}") for k in range(lstm.num_layers)
          for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    if any(t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t in ts):
        return None
    return (n_in, H, lstm.num_layers), ts


def _desc(meta, ts, grads=None) -> AgxLstmDesc:
    d = AgxLstmDesc()
    d.in_, d.H, d.L = meta
    for k in range(meta[2]):
        for j, n in enumerate(_LAYER_IN):
            setattr(d.layer[k], n, ts[4 * k + j].data_ptr())
            if grads is not None:
                setattr(d.layer[k], "g_" + n, grads[4 * k + j].data_ptr())
    return d


class LstmFn(torch.autograd.Function):
    """(x [B, T, in], h0, c0 [L, B, H], the nn.LSTM's parameters...) -> (y [B, T, H], h_n, c_n)."""

    @staticmethod
    def forward(ctx, meta, split, x, h0, c0, *ts):
        x, h0, c0 = x.contiguous(), h0.contiguous(), c0.contiguous()
        (B, T, _), (_, H, L) = x.shape, meta
        y = torch.empty(B, T, H, dtype=torch.float32, device=x.device)
        h_n, c_n = torch.empty_like(h0), torch.empty_like(c0)
        d = _desc(meta, ts)
        ctx.set_materialize_grads(False)  # an output without a cotangent reaches the backward as None, not zeros
        saved = ws = None
        if any(ctx.needs_input_grad):
            n = _lib.load().agx_lstm_saved_bytes(ctypes.byref(d), B, T)
            saved = torch.empty(n // 4, dtype=torch.float32, device=x.device)
        args = (ctypes.byref(d), x.data_ptr(), h0.data_ptr(), c0.data_ptr(), B, T, y.data_ptr(), h_n.data_ptr(),
                c_n.data_ptr(), _lib.ptr(saved))
        if split:  # one workspace, of the backward's size when a backward will follow, serves both
            nws = _lib.load().agx_lstm_split_workspace_bytes(ctypes.byref(d), B, T, int(saved is not None))
            ws = torch.empty(nws // 4, dtype=torch.float32, device=x.device)
            _lib.call("agx_lstm_forward_split", *args, ws.data_ptr(), _lib.stream())
        else:
            _lib.call("agx_lstm_forward", *args, _lib.stream())
        ctx.meta, ctx.ws = meta, ws
        if saved is not None:
            ctx.save_for_backward(x, h0, c0, y, saved, *ts)
        return y, h_n, c_n

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gh_n, gc_n):
        x, h0, c0, y, saved, *ts = ctx.saved_tensors
        B, T, _ = x.shape
        gy = torch.zeros_like(y) if gy is None else gy.to(torch.float32).contiguous()
        gh_n = None if gh_n is None else gh_n.to(torch.float32).contiguous()
        gc_n = None if gc_n is None else gc_n.to(torch.float32).contiguous()
        grads = [torch.empty_like(t) for t in ts]
        gx = torch.empty_like(x) if ctx.needs_input_grad[2] else None
        gh0 = torch.empty_like(h0) if ctx.needs_input_grad[3] else None
        gc0 = torch.empty_like(c0) if ctx.needs_input_grad[4] else None
        d = _desc(ctx.meta, ts, grads)
        ws = ctx.ws  # the split forward's, sized for its backward
        if ws is None:
            nws = _lib.load().agx_lstm_workspace_bytes(ctypes.byref(d), B, T)
            ws = torch.empty(nws // 4, dtype=torch.float32, device=x.device)
        _lib.call("agx_lstm_backward_split" if ctx.ws is not None else "agx_lstm_backward", ctypes.byref(d),
                  x.data_ptr(), h0.data_ptr(), c0.data_ptr(), B, T, y.data_ptr(), saved.data_ptr(), gy.data_ptr(),
                  _lib.ptr(gh_n), _lib.ptr(gc_n), _lib.ptr(gx), _lib.ptr(gh0), _lib.ptr(gc0), ws.data_ptr(),
                  _lib.stream())
        return (None, None, gx, gh0, gc0,
                *[g if ctx.needs_input_grad[5 + i] else None for i, g in enumerate(grads)])


def choose_plan(meta, B: int, T: int) -> str:
    """agx_lstm_choose_plan's form for (in, H, L) at B sequences of T steps: "whole" or "split"."""
    d, split = AgxLstmDesc(), ctypes.c_int32(0)
    d.in_, d.H, d.L = meta
    lib = _lib.load(require_gpu=False)
    _lib.check(lib.agx_lstm_choose_plan(ctypes.byref(d), B, T, ctypes.byref(split)), "agx_lstm_choose_plan")
    return "split" if split.value else "whole"


def lstm_sequence(module: EvolvableLSTM, x: torch.Tensor, h0: torch.Tensor, c0: torch.Tensor,
                  plan: str | None = None):
    """``module.lstm(x, (h0, c0))`` on the fused kernels as (y, h_n, c_n), or None where they do not apply.
    ``plan``: "whole", "split" or None (AGX_LSTM_PLAN, else the library's choice); the results do not depend on it."""
    plan = plan or os.environ.get("AGX_LSTM_PLAN") or None
    if plan not in (None, "whole", "split"):
        raise ValueError(f"lstm_sequence: plan {plan!r} is neither 'whole' nor 'split'")
    if not enabled() or not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
                                for t in (x, h0, c0)):
        return None
    found = _plan(module.lstm)
    if found is None or hooked(module):
        return None
    meta, ts = found
    n_in, H, L = meta
    if (x.dim() != 3 or x.shape[2] != n_in or min(x.shape[:2]) < 1 or x.shape[0] * x.shape[1] > _MAX_ROWS or
            tuple(h0.shape) != (L, x.shape[0], H) or tuple(c0.shape) != (L, x.shape[0], H)):
        return None
    if plan is None:
        plan = choose_plan(meta, x.shape[0], x.shape[1])
    return LstmFn.apply(meta, plan == "split", x, h0, c0, *ts)

"""Drop-in ``EvolvableSimBa`` (agilerl/modules/simba.py), ``create_simba``
(agilerl/utils/evolvable_networks.py:647-710) and ``SimbaResidualBlock``
(agilerl/modules/custom_components.py:224-261), with the encoder's forward
and backward on agx_simba_forward / _backward (include/agx_simba.h,
csrc/simba.hip).

Same constructor, module names (``{name}_linear_layer_input``,
``{name}_residual_block_{i}`` with ``layer_norm`` / ``linear1`` / ``linear2``,
``{name}_layer_norm_output``, ``{name}_linear_layer_output``,
``{name}_activation_output``) and initialisation calls in the reference's
order, so a seeded build has the reference's weights bit for bit.

``simba_encoder(module, x, plan=None)`` runs the whole encoder in blocks + 2
launches forward and blocks + 2 backward; the parameters stay the modules' own
tensors and gradients come back through autograd.  It applies to f32 CUDA
tensors of 1..1024 rows, widths (inputs, hidden, outputs) up to 512, an
inner width scale_factor * hidden up to 2048, 1..8 blocks and an output
activation of None / Identity / ReLU, on modules without hooks; anything else
keeps the torch modules.

A plan (S, R, Q) splits a block's launches beyond their 16-row tiles: S inner
slices, R row tiles per workgroup, Q row ranges of the dW role, the partial
tiles summed in a fixed order by the last workgroup to arrive
(include/agx_simba.h).  ``plan=None`` takes agx_simba_choose_plan's: (1, 1, 1),
the whole kernels, for at most 256 rows and scale_factor * hidden^2 up to
4 * 224^2, and the fastest plan of the sweep in DESIGN 4.12 elsewhere.
AGX_SIMBA_SPLIT=0 makes that choice (1, 1, 1) everywhere (A/B runs); a tuple
forces a plan and an illegal one raises ValueError.

``EvolvableSimBa.forward`` takes the fused path where it was measured faster
than the torch modules: at most 256 rows and scale_factor *
hidden^2 up to 4 * 224^2 on the whole kernels, and at most 64 rows up to
4 * 256^2 on the split ones.  Elsewhere the split kernels are 2 to 3.4 times
faster than the whole ones and still 1.2 to 4.9 times slower than torch, so
those shapes stay with torch.  AGX_SIMBA=1 takes the fused path wherever it
applies, AGX_SIMBA=0 never (the torch encoder, for A/B checks)."""

from __future__ import annotations

import copy
import ctypes
import os
from collections import OrderedDict
from typing import Any

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable
from torch.nn import functional as F

from .. import _lib
from ._hooks import hooked
from .mlp import get_activation, preserve_parameters

_MAX_BLOCKS, _MAX_ROWS, _MAX_WIDTH, _MAX_INNER = 8, 1024, 512, 2048
_AUTO_MAX_ROWS, _AUTO_MAX_WORK = 256, 4 * 224 * 224  # forward()'s own bounds: rows, scale_factor * hidden^2
_AUTO_SPLIT_MAX_ROWS, _AUTO_SPLIT_MAX_WORK = 64, 4 * 256 * 256  # and where the split plans were measured faster
_COUNTER_BYTES = 1024  # AGX_SIMBA_COUNTER_BYTES
_ACTS = {"Identity": 0, "ReLU": 1}
_BLOCK_IN = ("ln_g", "ln_b", "w1", "b1", "w2", "b2")
_TOP_IN = ("w_in", "b_in", "ln_g", "ln_b", "w_out", "b_out")


class AgxSimbaBlock(ctypes.Structure):
    """Mirror of ``agx_simba_block`` (include/agx_simba.h)."""

    _fields_ = [(n, ctypes.c_void_p) for n in _BLOCK_IN] + [("g_" + n, ctypes.c_void_p) for n in _BLOCK_IN]


class AgxSimbaPlan(ctypes.Structure):
    """Mirror of ``agx_simba_plan`` (include/agx_simba.h): inner slices S, row tiles per workgroup R,
    role-W row ranges Q."""

    _fields_ = [(n, ctypes.c_int32) for n in ("slices", "row_tiles", "w_parts")]


class AgxSimbaDesc(ctypes.Structure):
    """Mirror of ``agx_simba_desc`` (include/agx_simba.h)."""

    _fields_ = ([(n, ctypes.c_void_p) for n in _TOP_IN] + [("g_" + n, ctypes.c_void_p) for n in _TOP_IN] +
                [("blk", AgxSimbaBlock * _MAX_BLOCKS)] +
                [(n, ctypes.c_void_p) for n in ("acts", "stats", "out")] +
                [(n, ctypes.c_int32) for n in ("in_", "H", "scale", "blocks", "out_dim", "act")] +
                [("eps", ctypes.c_float)])


class SimbaResidualBlock(nn.Module):
    """x + linear2(relu(linear1(layer_norm(x)))), He-uniform linears."""

    def __init__(self, hidden_size: int, scale_factor: float = 4, device="cpu") -> None:
        super().__init__()
        self.hidden_size = hidden_size
        self.layer_norm = nn.LayerNorm(hidden_size, device=device)
        self.linear1 = nn.Linear(hidden_size, hidden_size * scale_factor, device=device)
        self.linear2 = nn.Linear(hidden_size * scale_factor, hidden_size, device=device)
        nn.init.kaiming_uniform_(self.linear1.weight)
        nn.init.kaiming_uniform_(self.linear2.weight)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x + self.linear2(F.relu(self.linear1(self.layer_norm(x))))


def create_simba(input_size: int, output_size: int, hidden_size: int, num_blocks: int,
                 output_activation: str | None = None, scale_factor: float = 4.0, device="cpu",
                 name: str = "simba") -> nn.Sequential:
    net: OrderedDict[str, nn.Module] = OrderedDict()
    net[f"{name}_linear_layer_input"] = nn.Linear(input_size, hidden_size, device=device)
    nn.init.orthogonal_(net[f"{name}_linear_layer_input"].weight)
    for i in range(1, num_blocks + 1):
        net[f"{name}_residual_block_{i}"] = SimbaResidualBlock(hidden_size, scale_factor=scale_factor, device=device)
    net[f"{name}_layer_norm_output"] = nn.LayerNorm(hidden_size, device=device)
    net[f"{name}_linear_layer_output"] = nn.Linear(hidden_size, output_size, device=device)
    nn.init.orthogonal_(net[f"{name}_linear_layer_output"].weight)
    net[f"{name}_activation_output"] = get_activation(output_activation)
    return nn.Sequential(net)


class EvolvableSimBa(nn.Module):
    LAYER_METHODS = ("add_block", "remove_block")
    NODE_METHODS = ("add_node", "remove_node")

    def __init__(self, num_inputs: int, num_outputs: int, hidden_size: int, num_blocks: int,
                 output_activation: str | None = None, scale_factor: int = 4, min_blocks: int = 1,
                 max_blocks: int = 4, min_mlp_nodes: int = 16, max_mlp_nodes: int = 500, device="cpu",
                 name: str = "simba", random_seed: int | None = None) -> None:
        super().__init__()
        assert isinstance(scale_factor, int), "Scale factor must be an integer."
        self.device, self.random_seed, self.name = device, random_seed, name
        self.rng = np.random.default_rng(seed=random_seed)
        self.num_inputs, self.num_outputs = num_inputs, num_outputs
        self.hidden_size, self.num_blocks = hidden_size, num_blocks
        self.output_activation, self.scale_factor = output_activation, scale_factor
        self.min_blocks, self.max_blocks = min_blocks, max_blocks
        self.min_mlp_nodes, self.max_mlp_nodes = min_mlp_nodes, max_mlp_nodes
        self.last_mutation_attr: str | None = None
        self.disabled: set[str] = set()
        self.model = self._create()

    def _create(self) -> nn.Sequential:
        return create_simba(input_size=self.num_inputs, output_size=self.num_outputs, hidden_size=self.hidden_size,
                            num_blocks=self.num_blocks, output_activation=self.output_activation,
                            scale_factor=self.scale_factor, device=self.device, name=self.name)

    @property
    def net_config(self) -> dict[str, Any]:
        """Constructor arguments minus num_inputs / num_outputs / device / name (simba.py:94-102)."""
        return dict(hidden_size=self.hidden_size, num_blocks=self.num_blocks,
                    output_activation=self.output_activation, scale_factor=self.scale_factor,
                    min_blocks=self.min_blocks, max_blocks=self.max_blocks, min_mlp_nodes=self.min_mlp_nodes,
                    max_mlp_nodes=self.max_mlp_nodes, random_seed=self.random_seed)

    @property
    def activation(self) -> str:
        return "ReLU"

    def forward(self, x) -> torch.Tensor:
        if not isinstance(x, torch.Tensor):
            x = torch.tensor(np.asarray(x), dtype=torch.float32, device=self.device)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        fused = simba_encoder(self, x) if _faster(self, x.shape[0]) else None
        return fused if fused is not None else self.model(x)

    def get_output_dense(self) -> nn.Module:
        return getattr(self.model, f"{self.name}_linear_layer_output")

    def init_weights_gaussian(self, std_coeff: float = 4, output_coeff: float = 4) -> None:
        from .mlp import EvolvableMLP

        EvolvableMLP._init_gaussian(self.model, std_coeff)
        EvolvableMLP._init_gaussian(self.get_output_dense(), output_coeff)

    def disable_mutations(self, kind: str | None = None) -> None:
        if kind in (None, "layer"):
            self.disabled.update(self.LAYER_METHODS)
        if kind in (None, "node"):
            self.disabled.update(self.NODE_METHODS)

    def change_activation(self, activation: str, output: bool = False) -> None:
        """SimBa keeps ReLU (simba.py:136-144)."""
        return

    # ---- architecture mutations (simba.py:146-222) --------------------------
    def add_block(self) -> dict[str, int] | None:
        self.last_mutation_attr = "add_block"
        if self.num_blocks < self.max_blocks:
            self.num_blocks += 1
            self.recreate_network()
            return None
        return self.add_node()

    def remove_block(self) -> dict[str, int] | None:
        self.last_mutation_attr = "remove_block"
        if self.num_blocks > self.min_blocks:
            self.num_blocks -= 1
            self.recreate_network()
            return None
        return self.add_node()

    def add_node(self, numb_new_nodes: int | None = None) -> dict[str, int]:
        self.last_mutation_attr = "add_node"
        if numb_new_nodes is None:
            numb_new_nodes = int(self.rng.choice([16, 32, 64]))
        if self.hidden_size + numb_new_nodes <= self.max_mlp_nodes:
            self.hidden_size += numb_new_nodes
        self.recreate_network()
        return {"numb_new_nodes": numb_new_nodes}

    def remove_node(self, numb_new_nodes: int | None = None) -> dict[str, int]:
        self.last_mutation_attr = "remove_node"
        if numb_new_nodes is None:
            numb_new_nodes = int(self.rng.choice([16, 32, 64]))
        if self.hidden_size - numb_new_nodes > self.min_mlp_nodes:
            self.hidden_size -= numb_new_nodes
        self.recreate_network()
        return {"numb_new_nodes": numb_new_nodes}

    def recreate_network(self) -> None:
        self.model = preserve_parameters(self.model, self._create())

    def clone(self) -> "EvolvableSimBa":
        return copy.deepcopy(self)


# ---- the fused path ---------------------------------------------------------
def enabled() -> bool:
    return os.environ.get("AGX_SIMBA", "1") != "0"


def _faster(module: EvolvableSimBa, rows: int) -> bool:
    """The shapes at which the fused path was measured faster, unless AGX_SIMBA=1 asks for it everywhere."""
    if os.environ.get("AGX_SIMBA") == "1":
        return True
    work = module.scale_factor * module.hidden_size ** 2
    if rows <= _AUTO_MAX_ROWS and work <= _AUTO_MAX_WORK:
        return True
    return (rows <= _AUTO_SPLIT_MAX_ROWS and work <= _AUTO_SPLIT_MAX_WORK and
            os.environ.get("AGX_SIMBA_SPLIT") != "0")


def _plan(module: EvolvableSimBa):
    """(meta, parameter tensors in descriptor order) of a create_simba stack, or None."""
    mods = list(module.model.children())
    if len(mods) < 5 or type(mods[0]) is not nn.Linear or type(mods[-3]) is not nn.LayerNorm \
            or type(mods[-2]) is not nn.Linear:
        return None
    blocks = mods[1:-3]
    act = _ACTS.get(type(mods[-1]).__name__)
    if act is None or not 1 <= len(blocks) <= _MAX_BLOCKS or any(type(b) is not SimbaResidualBlock for b in blocks):
        return None
    lin_in, ln_out, lin_out = mods[0], mods[-3], mods[-2]
    H, scale = lin_in.out_features, module.scale_factor
    if (not isinstance(scale, int) or scale < 1 or H > _MAX_WIDTH or scale * H > _MAX_INNER or
            lin_in.in_features > _MAX_WIDTH or lin_out.out_features > _MAX_WIDTH):
        return None
    ts = [lin_in.weight, lin_in.bias, ln_out.weight, ln_out.bias, lin_out.weight, lin_out.bias]
    eps = ln_out.eps
    for b in blocks:
        if b.layer_norm.eps != eps or b.linear1.out_features != scale * H:
            return None
        ts += [b.layer_norm.weight, b.layer_norm.bias, b.linear1.weight, b.linear1.bias, b.linear2.weight,
               b.linear2.bias]
    if any(t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() for t in ts):
        return None
    return (lin_in.in_features, H, scale, len(blocks), lin_out.out_features, act, float(eps)), ts


def _desc(meta, ts, acts, stats, out, grads=None) -> AgxSimbaDesc:
    d = AgxSimbaDesc()
    d.in_, d.H, d.scale, d.blocks, d.out_dim, d.act, d.eps = meta
    for j, n in enumerate(_TOP_IN):
        setattr(d, n, ts[j].data_ptr())
        if grads is not None:
            setattr(d, "g_" + n, grads[j].data_ptr())
    for i in range(meta[3]):
        for j, n in enumerate(_BLOCK_IN):
            k = 6 + 6 * i + j
            setattr(d.blk[i], n, ts[k].data_ptr())
            if grads is not None:
                setattr(d.blk[i], "g_" + n, grads[k].data_ptr())
    d.acts, d.stats, d.out = acts.data_ptr(), stats.data_ptr(), out.data_ptr()
    return d


class SimbaFn(torch.autograd.Function):
    """(x [B, in], the encoder's parameters...) -> [B, out].  ``plan``: None for agx_simba_forward /
    _backward, an (S, R, Q) tuple for the split entry points; the backward runs under the forward's plan."""

    @staticmethod
    def forward(ctx, meta, plan, x, *ts):
        x = x.contiguous()
        B, (_, H, _, blocks, nout, _, _) = x.shape[0], meta
        acts = torch.empty(blocks + 1, B, H, dtype=torch.float32, device=x.device)
        stats = torch.empty(blocks + 1, B, 2, dtype=torch.float32, device=x.device)
        out = torch.empty(B, nout, dtype=torch.float32, device=x.device)
        d = _desc(meta, ts, acts, stats, out)
        ctx.ws = None
        if plan is None:
            _lib.call("agx_simba_forward", ctypes.byref(d), x.data_ptr(), B, _lib.stream())
        else:
            # one workspace for both passes when a backward will follow: the counters are zero again after each
            ws = _split_workspace(d, B, plan, any(ctx.needs_input_grad), x.device)
            _lib.call("agx_simba_forward_split", ctypes.byref(d), x.data_ptr(), B, ctypes.byref(AgxSimbaPlan(*plan)),
                      ws.data_ptr(), _lib.stream())
            ctx.ws = ws if any(ctx.needs_input_grad) else None
        ctx.meta, ctx.plan = meta, plan
        ctx.save_for_backward(x, acts, stats, out, *ts)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, acts, stats, out, *ts = ctx.saved_tensors
        B = x.shape[0]
        g = g.to(torch.float32).contiguous()
        grads = [torch.empty_like(t) for t in ts]
        gx = torch.empty_like(x) if ctx.needs_input_grad[2] else None
        d = _desc(ctx.meta, ts, acts, stats, out, grads)
        if ctx.plan is None:
            nws = _lib.load().agx_simba_workspace_bytes(ctypes.byref(d), B)
            ws = torch.empty(max(16, nws), dtype=torch.uint8, device=x.device)
            _lib.call("agx_simba_backward", ctypes.byref(d), x.data_ptr(), B, g.data_ptr(), _lib.ptr(gx),
                      ws.data_ptr(), _lib.stream())
        else:
            ws = ctx.ws if ctx.ws is not None else _split_workspace(d, B, ctx.plan, True, x.device)
            _lib.call("agx_simba_backward_split", ctypes.byref(d), x.data_ptr(), B, g.data_ptr(), _lib.ptr(gx),
                      ctypes.byref(AgxSimbaPlan(*ctx.plan)), ws.data_ptr(), _lib.stream())
        return (None, None, gx, *[gr if ctx.needs_input_grad[3 + i] else None for i, gr in enumerate(grads)])


def _split_workspace(d: AgxSimbaDesc, B: int, plan, backward: bool, device) -> torch.Tensor:
    """The split entry points' workspace with its counter region zeroed (by a fill kernel, so that it can
    be captured); an illegal plan raises with the library's reason."""
    n = _lib.load().agx_simba_split_workspace_bytes(ctypes.byref(d), B, ctypes.byref(AgxSimbaPlan(*plan)),
                                                    int(backward))
    if n == 0:
        raise ValueError(f"simba plan {tuple(plan)}: {_lib.load().agx_last_error().decode(errors='replace')}")
    ws = torch.empty(n, dtype=torch.uint8, device=device)
    ws[:_COUNTER_BYTES].zero_()
    return ws


def choose_plan(meta, B: int):
    """The library's plan for this shape as (S, R, Q); (1, 1, 1) under AGX_SIMBA_SPLIT=0."""
    if os.environ.get("AGX_SIMBA_SPLIT") == "0":
        return (1, 1, 1)
    d, p = AgxSimbaDesc(), AgxSimbaPlan()
    d.in_, d.H, d.scale, d.blocks, d.out_dim, d.act, d.eps = meta
    _lib.check(_lib.load().agx_simba_choose_plan(ctypes.byref(d), B, ctypes.byref(p)), "agx_simba_choose_plan")
    return (p.slices, p.row_tiles, p.w_parts)


def simba_encoder(module: EvolvableSimBa, x: torch.Tensor, plan=None):
    """``module.model(x)`` on the fused kernels, or None where they do not apply.  ``plan``: None for the
    library's choice, or (S, R, Q) to force the split kernels' plan (include/agx_simba.h); an illegal one
    raises ValueError."""
    if (not enabled() or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or
            x.dim() != 2 or not 1 <= x.shape[0] <= _MAX_ROWS):
        return None
    found = _plan(module)
    if found is None or found[0][0] != x.shape[1] or hooked(module):
        return None
    meta, ts = found
    if plan is None:
        plan = choose_plan(meta, x.shape[0])
        plan = None if plan == (1, 1, 1) else plan  # the whole kernels' own entry points
    else:
        plan = tuple(int(v) for v in plan)
        if len(plan) != 3:
            raise ValueError(f"simba plan {plan}: not (S, R, Q)")
    return SimbaFn.apply(meta, plan, x, *ts)

"""Checkpoints in the layout of ``get_checkpoint_dict`` (agilerl/algorithms/
core/base.py:168-224, 939-1072): hyper-parameter attributes at the top level
plus ``network_info = {network_names, modules: {<net>_state_dict},
optimizer_names, optimizers: {<opt>_state_dict}}``, with the reference's
state-dict key names.

Differences of form: classes and spaces are not pickled (the file holds only
tensors, numbers, strings, lists and dicts), so it is written by
``torch.save`` and read back with ``torch.load(weights_only=True)`` — nothing
in a checkpoint is executed on load.  Spaces are stored as
``{"obs_shape", "n_actions"}`` (a Box action space: ``{"obs_shape",
"action_low", "action_high"}``, its bounds as flat lists; a MultiDiscrete
one: ``{"obs_shape", "nvec"}``; a MultiBinary one: ``{"obs_shape", "n_binary"}``)
for ``load``.

Checkpoints the reference itself wrote (dill-pickled agents, spaces and
registries) are read by ``refckpt.read_reference`` — the same weights-only
unpickler with inert stand-ins for the classes they name — and converted to
this layout, so ``load_checkpoint`` / ``load`` accept either file.
"""

from __future__ import annotations

import pickle
from typing import Any

import torch

HP_NAMES = ("index", "batch_size", "lr", "learn_step", "gamma", "tau", "double", "beta", "prior_eps", "num_atoms",
            "v_min", "v_max", "noise_std", "n_step", "combined_reward", "gae_lambda", "clip_coef", "ent_coef",
            "vf_coef", "max_grad_norm", "target_kl", "update_epochs", "num_envs", "net_config", "scores", "fitness",
            "steps", "mut", "normalize_images", "action_std_init")


def _plain(v: Any) -> Any:
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().clone()
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if hasattr(v, "item") and callable(v.item) and not isinstance(v, (str, bytes)):
        return v.item()
    return v


def checkpoint_dict(agent, modules: dict[str, dict[str, torch.Tensor]], optimizers: dict[str, Any],
                    spaces: bool = True) -> dict:
    out = {k: _plain(getattr(agent, k)) for k in HP_NAMES if hasattr(agent, k)}
    out["algo"] = agent.algo
    out["agilerl_version"] = "agx"
    if spaces:
        out["spaces"] = {"obs_shape": list(agent.observation_space.shape)}
        if hasattr(agent.action_space, "nvec"):  # MultiDiscrete actions (1-D)
            out["spaces"]["nvec"] = [int(n) for n in agent.action_space.nvec]
        elif type(agent.action_space).__name__ == "MultiBinary":  # n independent switches (1-D)
            out["spaces"]["n_binary"] = int(agent.action_space.n)
        elif hasattr(agent.action_space, "n"):
            out["spaces"]["n_actions"] = int(agent.action_space.n)
        else:  # Box actions (1-D)
            out["spaces"]["action_low"] = [float(x) for x in agent.action_space.low]
            out["spaces"]["action_high"] = [float(x) for x in agent.action_space.high]
    out["network_info"] = {
        "network_names": list(modules),
        "modules": {f"{k}_state_dict": _plain(v) for k, v in modules.items()},
        "optimizer_names": list(optimizers),
        "optimizers": {f"{k}_state_dict": _plain(v) for k, v in optimizers.items()},
    }
    return out


def load_file(path: str, adam_networks: tuple[str, ...] | None = None) -> dict:
    """An agx checkpoint as written, or a reference one converted to the agx
    layout (refckpt.to_agx; ``adam_networks`` as there)."""
    from . import refckpt

    try:
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError:
        ckpt = refckpt.read_reference(path)
    if isinstance(ckpt, dict) and ckpt.get("agilerl_version") == "agx":
        return ckpt
    if not refckpt.is_reference_checkpoint(ckpt):
        raise ValueError(f"{path}: not an agent checkpoint of agilerl >= 2.0 (no network_info)")
    return refckpt.to_agx(ckpt, adam_networks)


def read(path: str, algo: str, adam_networks: tuple[str, ...] | None = None) -> dict:
    ckpt = load_file(path, adam_networks)
    if ckpt.get("algo") != algo:
        raise ValueError("Loaded registry does not match the algorithm's registry. Please make sure you are "
                         "loading the checkpoint with the correct algorithm.")
    return ckpt


def restore_attributes(agent, ckpt: dict) -> None:
    for k in HP_NAMES:
        if k in ckpt:
            setattr(agent, k, ckpt[k])


def spaces(ckpt: dict):
    from ..envs import Box, Discrete, MultiBinary, MultiDiscrete

    s = ckpt["spaces"]
    obs = Box(-float("inf"), float("inf"), tuple(s["obs_shape"]))
    if "nvec" in s:
        return obs, MultiDiscrete(s["nvec"])
    if "n_binary" in s:
        return obs, MultiBinary(s["n_binary"])
    if "n_actions" not in s:
        act = Box(0.0, 0.0, (len(s["action_low"]),))
        act.low[:], act.high[:] = s["action_low"], s["action_high"]
        return obs, act
    return obs, Discrete(s["n_actions"])


def group_state_dicts(agent) -> tuple[dict, dict]:
    """(modules, optimizers): the state dicts of the agent's network groups
    (evolvable.py) by attribute name — net, target, net, target, ..., and the
    optimizers in group order; {agent id: state dict} for a dict-valued group."""
    def sd(x):
        return {a: m.state_dict() for a, m in x.items()} if hasattr(x, "items") else x.state_dict()

    return ({n: sd(getattr(agent, n)) for g in agent._groups for n in g[:2] if n},
            {g[2]: sd(getattr(agent, g[2])) for g in agent._groups})


def load_group_state_dicts(agent, info: dict) -> None:
    """``network_info`` into the agent's network groups.  An empty module
    state dict is skipped, as the reference (core/base.py:1006-1010)."""
    def load(x, sd, module):
        if hasattr(x, "items"):
            for a, s in sd.items():
                load(x[a], s, module)
        elif sd or not module:
            x.load_state_dict(sd)

    for g in agent._groups:
        for n in g[:2]:
            if n:  # a group without a target network names none
                load(getattr(agent, n), info["modules"].get(f"{n}_state_dict") or {}, True)
        load(getattr(agent, g[2]), info["optimizers"][f"{g[2]}_state_dict"], False)


class TorchCheckpointMixin:
    """save_checkpoint / load_checkpoint / load over the agent's network
    groups; what a class adds to the file goes through the two hooks."""

    _ckpt_spaces = True  # the file carries ``spaces``, so ``load`` can build the agent

    def _ckpt_extra(self, ck: dict) -> None:
        """Add the class's own top-level keys to a checkpoint being saved."""

    def _ckpt_restore(self, ck: dict) -> None:
        """Take them back, before the state dicts are loaded."""

    def save_checkpoint(self, path: str) -> None:
        ck = checkpoint_dict(self, *group_state_dicts(self), spaces=self._ckpt_spaces)
        self._ckpt_extra(ck)
        torch.save(ck, path)

    @torch.no_grad()
    def load_checkpoint(self, path: str) -> None:
        ck = read(path, self.algo)
        self._ckpt_restore(ck)
        load_group_state_dicts(self, ck["network_info"])
        restore_attributes(self, ck)

    @classmethod
    def load(cls, path: str, device="cuda", accelerator=None):
        ck = load_file(path)
        obs_space, act_space = spaces(ck)
        code = cls.__init__.__code__
        names = set(code.co_varnames[1:code.co_argcount])
        agent = cls(obs_space, act_space, device=device, **{k: ck[k] for k in names if k in ck})
        agent.load_checkpoint(path)
        return agent

"""Drop-in ``IPPO`` (agilerl/algorithms/ippo.py:46-956): independent PPO for
multi-agent environments with vector observations and Discrete, MultiDiscrete,
MultiBinary or Box actions.  Agents that share an id prefix (``listener_0``,
``listener_1``) share one actor and one critic.

Each network pair is one row of parameters in HBM: an actor-critic spec with
separate encoders (``share_encoders=False``, the reference's defaults: encoder
[64, 64] -> latent 32, actor head [32], critic head [64], ippo.py:291-327)
held by a one-agent ``PPOPopulation``, so the policy-step kernels and the
runtime-shape fused learner of PPO run it unchanged.  The learner's two clip
groups, [0, critic_start) and [critic_start, n_params), are the reference's
two ``clip_grad_norm_`` + Adam pairs.

``learn(experiences)`` per group: one upload of the assembled arrays, the
critic's value of ``next_state`` (one policy-step launch), ONE
``agx_ippo_gae`` launch for all groups (the float32 GAE of ippo.py:702-725,
bit for bit), the epochs' shuffles from numpy's global stream in the
reference's order, and the head's graph learner with
``adv_norm_minibatch = 1``: gather, per-minibatch normalisation
(ippo.py:780-783) and every epoch x minibatch update in three launches.  A
per-minibatch loop of the existing pieces (``_learn_loop``) runs instead when
``target_kl`` is set (the reference tests the epoch's last minibatch, the
learner the running mean), when a minibatch would hold one row, when the
network lies outside the graph learner's coverage, or with ``fused=False`` /
``AGX_IPPO_FUSED=0``; ``last_learn_paths`` records which ran.

Row order.  For a group of k > 1 agents the reference orders states and
actions as (agent, t, env) but log-probs, values, advantages and returns as
(t, agent, env), pairing a state with another transition's
advantage.  Here every transition keeps its own row: (t, agent, env) for all
eight arrays.

Outside this path: architecture mutations, inactive agents (NaN placeholders,
``agent_mask``), ``env_defined_actions``, Dict / Tuple / image observations,
custom ``actor_networks`` / ``critic_networks``, multi-rank populations;
``action_batch_size`` is accepted and ignored (a group's policy step is one
launch whatever its batch).
"""

from __future__ import annotations

import copy
import os
from collections import OrderedDict
from typing import Any

import numpy as np
import torch

from .. import _lib
from .. import kernels as K
from . import checkpoint as C

_HP = ("batch_size", "lr", "learn_step", "gamma", "gae_lambda", "clip_coef", "ent_coef", "vf_coef", "max_grad_norm",
       "target_kl", "update_epochs", "action_std_init")


def group_id(agent_id):
    """core/base.py:1824-1831: ``listener_0`` -> ``listener``."""
    return agent_id.rsplit("_", 1)[0] if isinstance(agent_id, str) else agent_id


def _as_dict(spaces, agent_ids) -> OrderedDict:
    if hasattr(spaces, "spaces"):
        spaces = spaces.spaces
    if hasattr(spaces, "keys"):
        return OrderedDict((a, spaces[a]) for a in agent_ids)
    return OrderedDict(zip(agent_ids, spaces))


def _same_space(a, b) -> bool:
    if type(a).__name__ != type(b).__name__ or tuple(getattr(a, "shape", ()) or ()) != tuple(getattr(b, "shape", ()) or ()):
        return False
    for name in ("n", "nvec", "low", "high"):
        if hasattr(a, name) != hasattr(b, name):
            return False
        if hasattr(a, name) and not np.array_equal(np.asarray(getattr(a, name)), np.asarray(getattr(b, name))):
            return False
    return True


def _stack(x) -> np.ndarray:
    """One agent's entry of an experience dict (a list of per-step arrays, an
    array or a tensor) as one numpy array with time leading."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy()
    if isinstance(x, (list, tuple)):
        return np.stack([v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in x])
    return np.asarray(x)


def assemble_rows(per_agent: dict, agents: list[str], num_steps: int | None, tail: tuple = ()) -> np.ndarray:
    """The (t, agent, env) layout of one experience array for a group:
    ``per_agent[a]`` [T, N, *tail] for every agent of ``agents`` (in the
    group's order) -> [T, k N, *tail], column a N + n agent a's env n — the
    order of ``vectorize_experiences_by_agent`` (stack(dim=1), reshape(T, -1)).
    ``num_steps`` None: a per-env array without the time axis ([N, *tail] ->
    [k N, *tail], the reference's ``dim=0`` form for next_state / next_done)."""
    arrs = [_stack(per_agent[a]) for a in agents]
    if num_steps is None:
        return np.concatenate([x.reshape(-1, *tail) for x in arrs], axis=0)
    return np.concatenate([x.reshape(num_steps, -1, *tail) for x in arrs], axis=1)


def disassemble(group_out: np.ndarray, agents: list[str], vect_dim: int, squeeze: bool) -> dict:
    """core/base.py:1868-1903 for one group: [k N, ...] -> {agent: [N, -1]},
    the last axis dropped when it is 1 and the action space Discrete."""
    out = np.reshape(group_out, (len(agents), vect_dim, -1))
    return {a: (out[i].squeeze(-1) if squeeze and out.shape[-1] == 1 else out[i]) for i, a in enumerate(agents)}


def _align(n: int) -> int:
    return (n + 15) // 16 * 16


class _NetView:
    """``agent.actors[gid]`` / ``agent.critics[gid]``: the network's tensors
    by the reference's state-dict names, as views of the group's HBM row."""

    def __init__(self, group, prefix: str):
        self.group, self.prefix = group, prefix + "."

    def _keys(self):
        spec = self.group.spec
        return {k[len(self.prefix):]: v for k, v in spec.state_dict_keys().items() if k.startswith(self.prefix)}

    def _views(self, flat: torch.Tensor) -> dict[str, torch.Tensor]:
        return OrderedDict((k, flat[off:off + int(np.prod(shape))].view(shape)) for k, (off, shape) in self._keys().items())

    def state_dict(self) -> dict[str, torch.Tensor]:
        return self._views(self.group.params.data[0])

    @torch.no_grad()
    def load_state_dict(self, sd: dict, strict: bool = True) -> None:
        own = self.state_dict()
        if strict and set(own) != set(sd):
            raise KeyError(f"state_dict mismatch: missing {sorted(set(own) - set(sd))}, unexpected "
                           f"{sorted(set(sd) - set(own))}")
        for k, t in own.items():
            if k in sd:
                t.copy_(torch.as_tensor(sd[k]).reshape(t.shape).to(t))

    def parameters(self):
        return list(self.state_dict().values())


def _make_group(spec, seed: int, device, hp: dict, fused: bool):
    """The one-agent population that holds a group's actor and critic."""
    from ..population.ppo_pop import PPOPopulation

    class Group(PPOPopulation):
        adv_norm_minibatch = True  # FusedLearner.learn: no adv_stats, the per-minibatch pass instead

        def resize(self, T: int, M: int) -> None:
            """Rollout storage for T steps of M = agents x envs columns: ONE
            byte buffer on the device (and its pinned host twin) that the
            arrays are views of, so a learn uploads once.  Reused while T and
            M stay the same."""
            if (T, M) == (self.T, self.N) and getattr(self, "stage_d", None) is not None:
                return
            self.T, self.N, self.S = int(T), int(M), int(T) * int(M)
            D, W = self.spec.obs_dim, self.act_width
            S = self.S
            act_bytes = S * W * (4 if self.gaussian else 8)
            sizes = [("obs", S * D * 4), ("actions", act_bytes), ("log_probs", S * 4), ("rewards", S * 4),
                     ("dones_f", S * 4), ("values", S * 4), ("next_obs", M * D * 4), ("next_done", M * 4)]
            offs, at = {}, 0
            for name, n in sizes:
                offs[name] = (at, n)
                at += _align(n)
            self.stage_h = torch.empty(max(at, 16), dtype=torch.uint8, pin_memory=True)
            self.stage_d = torch.empty(max(at, 16), dtype=torch.uint8, device=self.device)
            adt = torch.float32 if self.gaussian else torch.int64
            ashape = (1, T, M, W) if (self.gaussian or self.vector_int) else (1, T, M)
            shapes = {"obs": (torch.float32, (1, T, M, D)), "actions": (adt, ashape),
                      "log_probs": (torch.float32, (1, T, M)), "rewards": (torch.float32, (1, T, M)),
                      "dones_f": (torch.float32, (1, T, M)), "values": (torch.float32, (1, T, M)),
                      "next_obs": (torch.float32, (1, M, D)), "next_done": (torch.float32, (M,))}
            self.host = {}
            for name, (dt, shape) in shapes.items():
                o, n = offs[name]
                setattr(self, name, self.stage_d[o:o + n].view(dt).view(shape))
                self.host[name] = self.stage_h[o:o + n].view(dt).view(shape).numpy()
            f32 = dict(dtype=torch.float32, device=self.device)
            self.advantages = torch.zeros(1, T, M, **f32)
            self.returns = torch.zeros(1, T, M, **f32)
            self.next_value = torch.zeros(M, **f32)
            self.action_masks = None
            self._fused = None    # the learner's workspace is sized by S
            self._act_ws = None   # the policy step's by N
            self._rederive()

    hp = dict(hp)
    pop = Group(spec, 1, 1, learn_step=1, seeds=[seed], device=device, fused=fused, multi_fused=True, **hp)
    pop.stage_d = None
    return pop


class IPPO(C.TorchCheckpointMixin):
    algo = "IPPO"
    _ckpt_spaces = False  # the spaces of every agent go into the file through _ckpt_extra
    can_mutate_architecture = False  # recorded as "None" (hpo/mutation.py), as sharded off-policy agents are

    def __init__(self, observation_spaces, action_spaces, agent_ids: list[str] | None = None, index: int = 0,
                 hp_config=None, net_config: dict[str, Any] | None = None, batch_size: int = 64, lr: float = 1e-4,
                 learn_step: int = 2048, gamma: float = 0.99, gae_lambda: float = 0.95, mut: str | None = None,
                 action_std_init: float = 0.0, clip_coef: float = 0.2, ent_coef: float = 0.01, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, target_kl: float | None = None, normalize_images: bool = True,
                 update_epochs: int = 4, actor_networks=None, critic_networks=None,
                 action_batch_size: int | None = None, device="cuda", accelerator=None, torch_compiler=None,
                 wrap: bool = True, *, fused: bool = True) -> None:
        assert learn_step >= 1, "Learn step must be greater than or equal to one."
        assert isinstance(learn_step, int), "Learn step rate must be an integer."
        assert isinstance(batch_size, int), "Batch size must be an integer."
        assert batch_size >= 1, "Batch size must be greater than or equal to one."
        assert isinstance(lr, float), "Learning rate must be a float."
        assert lr > 0, "Learning rate must be greater than zero."
        assert isinstance(gamma, (float, int, torch.Tensor)), "Gamma must be a float."
        assert isinstance(gae_lambda, (float, int)), "Lambda must be a float."
        assert gae_lambda >= 0, "Lambda must be greater than or equal to zero."
        assert isinstance(action_std_init, (float, int)) and action_std_init >= 0, \
            "Action standard deviation must be greater than or equal to zero."
        assert isinstance(clip_coef, (float, int)) and clip_coef >= 0, \
            "Clipping coefficient must be greater than or equal to zero."
        assert isinstance(ent_coef, (float, int)) and ent_coef >= 0, \
            "Entropy coefficient must be greater than or equal to zero."
        assert isinstance(vf_coef, (float, int)) and vf_coef >= 0, \
            "Value function coefficient must be greater than or equal to zero."
        assert isinstance(max_grad_norm, (float, int)) and max_grad_norm >= 0, \
            "Maximum norm for gradient clipping must be greater than or equal to zero."
        assert isinstance(target_kl, (float, int)) or target_kl is None, \
            "Target KL divergence threshold must be a float."
        if target_kl is not None:
            assert target_kl >= 0, "Target KL divergence threshold must be greater than or equal to zero."
        assert isinstance(update_epochs, int) and update_epochs >= 1, \
            "Policy update epochs must be greater than or equal to one."
        assert isinstance(wrap, bool), "Wrap models flag must be boolean value True or False."
        if actor_networks is not None or critic_networks is not None:
            raise NotImplementedError("custom actor / critic modules: use net_config (MLP) networks")
        if accelerator is not None:
            raise NotImplementedError("agx IPPO: no accelerator (single process, DESIGN section 7)")
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise NotImplementedError("agx IPPO: multi-rank populations are not supported")
        if torch.device(device).type != "cuda":
            raise NotImplementedError(f"agx IPPO needs a ROCm device (got {device!r}): its networks live in HBM and "
                                      "act and learn through HIP kernels; of the multi-agent algorithms only MADDPG "
                                      "and MATD3 have a CPU path")
        from ..hpo.registry import MutationRegistry

        self._setup_agents(observation_spaces, action_spaces, agent_ids)
        self.index, self.hp_config, self.mut = index, hp_config, mut
        self.net_config = net_config
        self.batch_size, self.lr, self.learn_step = batch_size, lr, learn_step
        self.gamma, self.gae_lambda = gamma, gae_lambda
        self.action_std_init = action_std_init
        self.clip_coef, self.ent_coef, self.vf_coef = clip_coef, ent_coef, vf_coef
        self.max_grad_norm, self.target_kl = max_grad_norm, target_kl
        self.update_epochs = update_epochs
        self.normalize_images = normalize_images
        self.action_batch_size = action_batch_size
        self.torch_compiler = None
        self.accelerator = None
        self.fused = bool(fused)
        self.device = torch.device(device)
        self.registry = MutationRegistry(hp_config)
        self.scores: list = []
        self.fitness: list = []
        self.steps: list[int] = [0]
        self.training = True
        self.sharded = False
        self.last_learn_paths: dict[str, str] = {}
        self._build_networks()

    # ---- agents and groups (core/base.py:1426-1477) ------------------------------
    def _setup_agents(self, observation_spaces, action_spaces, agent_ids) -> None:
        if agent_ids is None:
            spaces = getattr(observation_spaces, "spaces", observation_spaces)
            agent_ids = list(spaces.keys()) if hasattr(spaces, "keys") else \
                [f"agent_{i}" for i in range(len(spaces))]
        self.agent_ids = list(agent_ids)
        self.possible_observation_spaces = _as_dict(observation_spaces, self.agent_ids)
        self.possible_action_spaces = _as_dict(action_spaces, self.agent_ids)
        self.shared_agent_ids: list[str] = []
        self.grouped_agents: dict[str, list[str]] = OrderedDict()
        self.unique_observation_spaces, self.unique_action_spaces = OrderedDict(), OrderedDict()
        for a in self.agent_ids:
            g = group_id(a)
            if g not in self.grouped_agents:
                self.shared_agent_ids.append(g)
                self.grouped_agents[g] = []
                self.unique_observation_spaces[g] = self.possible_observation_spaces[a]
                self.unique_action_spaces[g] = self.possible_action_spaces[a]
            assert _same_space(self.possible_observation_spaces[a], self.unique_observation_spaces[g]), \
                f"Homogeneous agents, i.e. agents that share the prefix {g}, must have the same observation space."
            assert _same_space(self.possible_action_spaces[a], self.unique_action_spaces[g]), \
                f"Homogeneous agents, i.e. agents that share the prefix {g}, must have the same action space."
            self.grouped_agents[g].append(a)
        self.n_unique_agents = len(self.shared_agent_ids)
        if self.has_grouped_agents():
            self.observation_space, self.action_space = self.unique_observation_spaces, self.unique_action_spaces
        else:
            self.observation_space, self.action_space = self.possible_observation_spaces, self.possible_action_spaces
        for g, s in self.observation_space.items():
            if not hasattr(s, "shape") or s.shape is None or len(s.shape) != 1:
                raise NotImplementedError(f"agx IPPO: 1-D vector observations (agent {g!r}: "
                                          f"{type(s).__name__} {getattr(s, 'shape', None)})")

    def has_grouped_agents(self) -> bool:
        return len(self.shared_agent_ids) < len(self.agent_ids)

    def get_group_id(self, agent_id):
        return group_id(agent_id)

    def get_network_id(self, agent_id):
        return group_id(agent_id) if self.has_grouped_agents() else agent_id

    def _members(self, net_id: str) -> list[str]:
        """The agents a network serves, in the reference's order."""
        return list(self.grouped_agents[net_id]) if self.has_grouped_agents() else [net_id]

    # ---- networks -----------------------------------------------------------------
    def _net_config_of(self, net_id: str) -> dict | None:
        """build_net_config(net_config, flatten=False) for one network: None,
        one single-level config for every network, or a dict keyed by agent /
        group ids."""
        cfg = self.net_config
        if cfg is None:
            return None
        keys = set(self.agent_ids) | set(self.shared_agent_ids)
        if any(k in keys for k in cfg):
            for k in (net_id, *self._members(net_id), group_id(net_id)):
                if k in cfg:
                    return cfg[k]
            return None
        return cfg

    def _build_networks(self) -> None:
        import dataclasses

        from .ppo import spec_from_net_config

        hp = {k: getattr(self, k) for k in _HP if k not in ("learn_step", "action_std_init")}
        self.groups: dict[str, Any] = OrderedDict()
        for j, g in enumerate(self.observation_space):
            cfg = self._net_config_of(g)
            spec = spec_from_net_config(self.observation_space[g], self.action_space[g], cfg, self.normalize_images,
                                        share_encoders=False, action_std_init=self.action_std_init)
            if cfg is None or cfg.get("head_config") is None:
                # ippo.py:301-306: the critic's default head is MlpNetConfig [64], not PPO's [16]
                spec = dataclasses.replace(spec, critic_hidden=[64], critic_limits=(1, 3, 16, 500))
            self.groups[g] = _make_group(spec, 1009 * int(self.index) + j, self.device, hp, self.fused)

    @property
    def actors(self) -> dict[str, _NetView]:
        return OrderedDict((g, _NetView(p, "actor")) for g, p in self.groups.items())

    @property
    def critics(self) -> dict[str, _NetView]:
        return OrderedDict((g, _NetView(p, "critic")) for g, p in self.groups.items())

    def set_training_mode(self, training: bool) -> None:
        self.training = bool(training)

    # ---- acting (ippo.py:497-597) ---------------------------------------------------
    def _masks(self, infos, net_id: str, members: list[str]):
        if infos is None:
            return None
        masks = [infos.get(a, {}).get("action_mask") if isinstance(infos.get(a), dict) else None for a in members]
        if all(m is None for m in masks):
            return None
        assert all(m is not None for m in masks), \
            "If action masks are provided for any agents, they must be provided for all agents."
        return masks

    @torch.no_grad()
    def _group_step(self, net_id: str, obs: np.ndarray, mask: np.ndarray | None, sample: bool = True):
        """One policy-step launch for a group: obs [M, D] (mask uint8 [M, L]
        or None) -> numpy (actions [M] or [M, W], log_prob, entropy, value [M])."""
        from ..population.learner import policy_step_graph

        pop = self.groups[net_id]
        M, D = obs.shape
        pop.resize(pop.T, M)
        obs_d = torch.as_tensor(obs, dtype=torch.float32).to(self.device).view(1, M, D).contiguous()
        mask_d = None if mask is None else torch.as_tensor(mask != 0).to(torch.uint8).to(self.device).contiguous()
        pop.act_counter += 1
        if pop.head is not None:
            action, logp, ent, value = pop._head_step(obs_d, sample=sample, counter=pop.act_counter,
                                                      action_mask=mask_d)
            action = action.view(M, -1)
        else:
            desc = pop.learn_descriptor()
            if desc is None:
                raise _lib.AgxError("agx_ppo_act_graph does not take this network: " +
                                    _lib.load(require_gpu=False).agx_last_error().decode(errors="replace"))
            action = torch.empty(1, M, dtype=torch.int64, device=self.device)
            logp, ent, value = (torch.empty(1, M, dtype=torch.float32, device=self.device) for _ in range(3))
            policy_step_graph(pop, desc, obs_d, M * D, sample=sample, counter=pop.act_counter, actions=action,
                              log_probs=logp, values=value, entropy=ent, out_agent_stride=M, action_mask=mask_d,
                              mask_agent_stride=M * pop.spec.n_actions)
            action = action.view(M)
        rest = torch.stack([logp.view(M), ent.view(M), value.view(M)]).cpu().numpy()
        return action.cpu().numpy(), rest[0], rest[1], rest[2]

    def get_action(self, obs: dict, infos: dict | None = None, *args, **kwargs):
        """-> (action, log_prob, entropy, value) dicts by agent id: the agents
        of a group batched agent-major into one policy-step launch."""
        for info in (infos or {}).values():
            if isinstance(info, dict) and info.get("env_defined_actions") is not None:
                raise NotImplementedError("agx IPPO: env_defined_actions are not supported")
        present = OrderedDict()
        for a in obs:
            present.setdefault(self.get_network_id(a), []).append(a)
        outs: tuple[dict, dict, dict, dict] = ({}, {}, {}, {})
        for net_id, members in present.items():
            space = self.action_space[net_id]
            D = int(np.prod(self.observation_space[net_id].shape))
            per = [np.asarray(obs[a], dtype=np.float32).reshape(-1, D) for a in members]
            vect_dim = per[0].shape[0]
            masks = self._masks(infos, net_id, members)
            mask = None if masks is None else np.concatenate(
                [np.asarray(m).reshape(vect_dim, -1) for m in masks], axis=0)
            action, logp, ent, value = self._group_step(net_id, np.concatenate(per, axis=0), mask)
            if not self.training and hasattr(space, "low") and not hasattr(space, "n"):
                action = np.clip(action, space.low, space.high)  # ippo.py:551-555
            if type(space).__name__ == "MultiBinary":
                action = action.astype(space.dtype)
            squeeze = type(space).__name__ == "Discrete"
            for out, arr in zip(outs, (action, logp, ent, value)):
                out.update(disassemble(arr, members, vect_dim, squeeze))
        return outs

    # ---- learning (ippo.py:599-836) -------------------------------------------------
    def _sync_hparams(self, pop) -> None:
        """The agent's (HPO-mutable) hyperparameters into a group's population."""
        if pop.agent_batch[0] != int(self.batch_size):
            pop.set_agent_hparam(0, "batch_size", int(self.batch_size))
        if pop.agent_epochs[0] != int(self.update_epochs):
            pop.set_agent_hparam(0, "update_epochs", int(self.update_epochs))
        if pop.agent_ent[0] != float(self.ent_coef):
            pop.set_agent_hparam(0, "ent_coef", float(self.ent_coef))
        if pop.agent_lr[0] != float(self.lr):
            pop.set_agent_hparam(0, "lr", float(self.lr))
        pop.ent_coef = float(self.ent_coef)
        pop.clip_coef, pop.vf_coef = float(self.clip_coef), float(self.vf_coef)
        pop.max_grad_norm = pop.opt.max_norm = float(self.max_grad_norm)
        pop.target_kl = self.target_kl
        pop.gamma, pop.gae_lambda = float(self.gamma), float(self.gae_lambda)

    def _fused_ok(self, pop) -> bool:
        if not self.fused or os.environ.get("AGX_IPPO_FUSED") == "0" or self.target_kl is not None:
            return False
        bb = min(int(self.batch_size), pop.S)
        if bb <= 1 or pop.S % bb == 1:
            return False  # a one-row minibatch: the reference skips it, the learner has no unbiased std for it
        return pop._fused_learner()

    def _upload(self, pop, net_id: str, members: list[str], exp) -> None:
        states, actions, log_probs, rewards, dones, values, next_states, next_dones = exp
        T = _stack(rewards[members[0]]).shape[0]
        N = int(_stack(rewards[members[0]]).reshape(T, -1).shape[1])
        pop.resize(T, N * len(members))
        D, W = pop.spec.obs_dim, pop.act_width
        h = pop.host
        h["obs"][0] = assemble_rows(states, members, T, (D,))
        a = assemble_rows(actions, members, T, (W,))
        h["actions"][0] = a if (pop.gaussian or pop.vector_int) else a[..., 0]
        for name, src in (("log_probs", log_probs), ("rewards", rewards), ("dones_f", dones), ("values", values)):
            h[name][0] = assemble_rows(src, members, T)
        h["next_obs"][0] = assemble_rows(next_states, members, None, (D,))
        h["next_done"][:] = assemble_rows(next_dones, members, None).reshape(-1)
        pop.stage_d.copy_(pop.stage_h, non_blocking=True)  # the one upload

    @torch.no_grad()
    def _bootstrap(self, pop) -> None:
        """next_value <- the critic's value of next_state (ippo.py:701): the
        group's policy-step kernel, values only."""
        from ..population.learner import policy_step_graph

        M, D = pop.N, pop.spec.obs_dim
        value = pop.next_value.view(1, M)
        if pop.head is not None:
            from ..population.learner import policy_step_head

            policy_step_head(pop, pop.next_obs, M * D, sample=False, counter=0, values=value, out_agent_stride=M)
            return
        desc = pop.learn_descriptor()
        if desc is None:
            _, v = pop.spec.forward(pop.params.data, pop.next_obs)
            value.copy_(v)
            return
        policy_step_graph(pop, desc, pop.next_obs, M * D, sample=False, counter=0, values=value, out_agent_stride=M)

    def learn(self, experiences) -> dict[str, float]:
        """One IPPO update from the 8-tuple of per-agent dicts (states, actions,
        log_probs, rewards, dones, values, next_state, next_done) ->
        {network id: mean loss} (ippo.py:835's mean_loss / (S * epochs))."""
        from ..population.learner import fused_learn
        from ..population.perms import draw_host_perms

        states = experiences[0]
        present = OrderedDict((g, [a for a in self._members(g) if a in states]) for g in self.observation_space)
        present = OrderedDict((g, m) for g, m in present.items() if m)
        segments = []
        for g, members in present.items():
            pop = self.groups[g]
            self._sync_hparams(pop)
            self._upload(pop, g, members, experiences)
            self._bootstrap(pop)
            segments.append((pop.rewards[0], pop.dones_f[0], pop.values[0], pop.next_value, pop.next_done,
                             pop.advantages[0], pop.returns[0]))
        for k in range(0, len(segments), K.IPPO_MAX_SEGMENTS):  # one launch for up to 8 groups
            K.ippo_gae(segments[k:k + K.IPPO_MAX_SEGMENTS], float(self.gamma), float(self.gae_lambda))
        out, fused_losses = {}, {}
        self.last_learn_paths = {}
        for g in present:
            pop = self.groups[g]
            if self._fused_ok(pop):
                E = int(self.update_epochs)
                host = np.empty((E, 1, pop.S), dtype=np.int64)
                draw_host_perms(host, [E], False, 1)  # E np.random.shuffle draws, this group's in turn
                perms = torch.from_numpy(host).to(self.device)
                fused_losses[g] = (fused_learn(pop, perms), perms)
                self.last_learn_paths[g] = "fused"
            else:
                out[g] = self._learn_loop(pop)
                self.last_learn_paths[g] = "loop"
        for g, (loss, _perms) in fused_losses.items():
            out[g] = float(loss[0].item())
            self.groups[g].check_errors()
        return {str(g): out[g] for g in present}

    def _learn_loop(self, pop) -> float:
        """_learn_individual's epochs (ippo.py:739-836) from the device arrays,
        minibatch by minibatch: torch autograd over the row, the two-group
        clip + Adam as one agx_clip_adam launch."""
        from ..population.nets import bernoulli_head, categorical, gaussian, multi_categorical

        spec, S = pop.spec, pop.S
        obs_f = pop.obs.view(S, spec.obs_dim)
        act_f = pop.actions.view(S, -1) if (pop.gaussian or pop.vector_int) else pop.actions.view(S)
        lp_f, adv_f = pop.log_probs.view(S), pop.advantages.view(S)
        ret_f, val_f = pop.returns.view(S), pop.values.view(S)
        idxs = np.arange(S)
        clip, vf, ent = float(self.clip_coef), float(self.vf_coef), float(self.ent_coef)
        total = torch.zeros((), dtype=torch.float64, device=self.device)
        approx_kl = None
        for _ in range(int(self.update_epochs)):
            np.random.shuffle(idxs)
            for start in range(0, S, int(self.batch_size)):
                mb = idxs[start:start + int(self.batch_size)]
                if len(mb) <= 1:
                    continue
                sel = torch.as_tensor(mb, device=self.device)
                w = pop.params.data.detach().clone().requires_grad_(True)
                logits, value = spec.forward(w, obs_f[sel].unsqueeze(0))
                if pop.gaussian:
                    logp, entropy = gaussian(logits[0], spec.log_std_view(w), act_f[sel])
                elif pop.multidiscrete:
                    logp, entropy = multi_categorical(logits[0], spec.nvec, act_f[sel])
                elif pop.multibinary:
                    logp, entropy = bernoulli_head(logits[0], act_f[sel])
                else:
                    logp_all, entropy = categorical(logits[0])
                    logp = logp_all.gather(-1, act_f[sel].unsqueeze(-1)).squeeze(-1)
                logratio = logp - lp_f[sel]
                ratio = logratio.exp()
                with torch.no_grad():
                    approx_kl = ((ratio - 1) - logratio).mean()
                a = adv_f[sel]
                a = (a - a.mean()) / (a.std() + 1e-8)
                pg_loss = torch.max(-a * ratio, -a * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
                v = value[0].view(-1)
                v_clipped = val_f[sel] + torch.clamp(v - val_f[sel], -clip, clip)
                v_loss = 0.5 * torch.max((v - ret_f[sel]) ** 2, (v_clipped - ret_f[sel]) ** 2).mean()
                actor_loss = pg_loss - ent * entropy.mean()
                critic_loss = v_loss * vf
                (actor_loss + critic_loss).backward()  # disjoint parameters: each loss's own gradient
                pop.opt.grads.copy_(w.grad)
                pop.opt.step()
                total += actor_loss.detach().double() + critic_loss.detach().double()
            if self.target_kl is not None and approx_kl is not None and float(approx_kl) > self.target_kl:
                break
        return float(total.item()) / (S * int(self.update_epochs))

    # ---- evaluation (ippo.py:838-956) -----------------------------------------------
    def sum_shared_rewards(self, rewards: dict) -> dict:
        first = next(iter(rewards.values()))
        shape = first.shape if isinstance(first, np.ndarray) else (1,)
        out = {g: np.zeros(shape) for g in self.shared_agent_ids}
        for a, r in rewards.items():
            out[group_id(a)] += r
        return out

    def test(self, env, swap_channels: bool = False, max_steps: int | None = None, loop: int = 3,
             sum_scores: bool = True):
        self.set_training_mode(False)
        try:
            vec = hasattr(env, "num_envs")
            num_envs = env.num_envs if vec else 1
            width = 1 if sum_scores else len(self.observation_space)
            rewards = []
            for _ in range(loop):
                obs, info = env.reset()
                scores = np.zeros((num_envs, width))
                completed = np.zeros((num_envs, width))
                finished = np.zeros(num_envs)
                step = 0
                while not np.all(finished):
                    step += 1
                    action, _, _, _ = self.get_action(obs=obs, infos=info)
                    if not vec:
                        action = {a: act[0] for a, act in action.items()}
                    obs, reward, term, trunc, info = env.step(action)
                    reward = self.sum_shared_rewards(reward)
                    r = np.array(list(reward.values())).transpose()
                    r = np.where(np.isnan(r), 0, r)
                    scores += ((np.sum(r, axis=-1)[:, None] if vec else np.sum(r, axis=-1)) if sum_scores else r)
                    dones = {}
                    for a in self.agent_ids:
                        t, u = term.get(a, True), trunc.get(a, False)
                        t = np.where(np.isnan(t), True, t).astype(bool)
                        u = np.where(np.isnan(u), False, u).astype(bool)
                        dones[a] = t | u
                    if not vec:
                        dones = {a: np.array([dones[a]]) for a in self.agent_ids}
                    for idx, agent_dones in enumerate(zip(*dones.values())):
                        if (np.all(agent_dones) or (max_steps is not None and step == max_steps)) \
                                and not finished[idx]:
                            completed[idx] = scores[idx]
                            finished[idx] = 1
                rewards.append(np.mean(completed, axis=0))
        finally:
            self.set_training_mode(True)
        mean_fit = np.mean(rewards, axis=0)
        mean_fit = mean_fit[0] if sum_scores else mean_fit
        self.fitness.append(mean_fit)
        return float(mean_fit) if sum_scores else mean_fit

    # ---- HPO hooks (hpo/mutation.py) ------------------------------------------------
    def get_lr_names(self) -> list[str]:
        return ["lr"]

    def reinit_optimizers(self, optimizer=None) -> None:
        """core/base.py:760-775: fresh Adams (zero moments and steps, the current lr)."""
        for pop in self.groups.values():
            pop.reinit_agent_optimizer(0)
            self._sync_hparams(pop)

    def policy_weight_groups(self) -> list[dict[str, torch.Tensor]]:
        """Each actor's weights by the reference's names, in network order
        (the ModuleDict policy of mutation.py:515-570)."""
        return [net.state_dict() for net in self.actors.values()]

    def mutation_hook(self) -> None:
        """Nothing is shared between an IPPO agent's networks."""

    # ---- clones and checkpoints -----------------------------------------------------
    def _ctor_args(self) -> dict:
        kw = {k: getattr(self, k) for k in _HP}
        kw.update(agent_ids=list(self.agent_ids), net_config=copy.deepcopy(self.net_config), mut=self.mut,
                  normalize_images=self.normalize_images, action_batch_size=self.action_batch_size,
                  device=self.device, fused=self.fused)
        return kw

    @torch.no_grad()
    def clone(self, index: int | None = None, wrap: bool = True) -> "IPPO":
        """EvolvableAlgorithm.clone (core/base.py): a new agent with this
        one's networks, Adam state, hyperparameters and history."""
        c = type(self)(self.possible_observation_spaces, self.possible_action_spaces,
                       index=self.index if index is None else index, hp_config=self.hp_config, **self._ctor_args())
        c.registry = copy.deepcopy(self.registry)
        for g, pop in self.groups.items():
            q = c.groups[g]
            q.params.data.copy_(pop.params.data)
            q.opt.exp_avg.copy_(pop.opt.exp_avg)
            q.opt.exp_avg_sq.copy_(pop.opt.exp_avg_sq)
            q.opt.steps.copy_(pop.opt.steps)
        c.scores, c.fitness, c.steps = list(self.scores), list(self.fitness), list(self.steps)
        return c

    def _adam_state(self, pop, prefix: str) -> dict:
        view = _NetView(pop, prefix)
        return {"exp_avg": view._views(pop.opt.exp_avg[0]), "exp_avg_sq": view._views(pop.opt.exp_avg_sq[0]),
                "step": int(pop.opt.steps[0]), "lr": float(self.lr)}

    def save_checkpoint(self, path: str) -> None:
        """core/base.py:939-949 in checkpoint.py's layout: ``actors`` and
        ``critics`` {network id: state dict}, ``actor_optimizers`` and
        ``critic_optimizers`` {network id: Adam state}."""
        mods = {"actors": {g: v.state_dict() for g, v in self.actors.items()},
                "critics": {g: v.state_dict() for g, v in self.critics.items()}}
        opts = {"actor_optimizers": {g: self._adam_state(p, "actor") for g, p in self.groups.items()},
                "critic_optimizers": {g: self._adam_state(p, "critic") for g, p in self.groups.items()}}
        ck = C.checkpoint_dict(self, mods, opts, spaces=False)
        ck["agent_ids"] = list(self.agent_ids)
        ck["agent_spaces"] = {a: self._space_record(a) for a in self.agent_ids}
        torch.save(ck, path)

    def _space_record(self, a: str) -> dict:
        act = self.possible_action_spaces[a]
        rec = {"obs_shape": [int(x) for x in self.possible_observation_spaces[a].shape]}
        if hasattr(act, "nvec"):
            rec["nvec"] = [int(n) for n in act.nvec]
        elif type(act).__name__ == "MultiBinary":
            rec["n_binary"] = int(act.n)
        elif hasattr(act, "n"):
            rec["n_actions"] = int(act.n)
        else:
            rec["action_low"] = [float(x) for x in np.asarray(act.low).reshape(-1)]
            rec["action_high"] = [float(x) for x in np.asarray(act.high).reshape(-1)]
        return rec

    @torch.no_grad()
    def load_checkpoint(self, path: str) -> None:
        ck = C.read(path, self.algo)
        info = ck["network_info"]
        for name, prefix, opt_name in (("actors", "actor", "actor_optimizers"),
                                       ("critics", "critic", "critic_optimizers")):
            for g, sd in info["modules"][f"{name}_state_dict"].items():
                pop = self.groups[g]
                view = _NetView(pop, prefix)
                view.load_state_dict(sd)
                st = info["optimizers"][f"{opt_name}_state_dict"][g]
                for which, flat in (("exp_avg", pop.opt.exp_avg[0]), ("exp_avg_sq", pop.opt.exp_avg_sq[0])):
                    for k, t in view._views(flat).items():
                        t.copy_(torch.as_tensor(st[which][k]).reshape(t.shape).to(t))
                pop.opt.steps[0] = int(st["step"])
        C.restore_attributes(self, ck)
        for pop in self.groups.values():
            self._sync_hparams(pop)

    @classmethod
    def load(cls, path: str, device="cuda", accelerator=None) -> "IPPO":
        ck = C.load_file(path)
        ids = list(ck["agent_ids"])
        obs, act = OrderedDict(), OrderedDict()
        for a in ids:
            obs[a], act[a] = C.spaces({"spaces": ck["agent_spaces"][a]})
        code = cls.__init__.__code__
        names = set(code.co_varnames[1:code.co_argcount]) - {"observation_spaces", "action_spaces", "agent_ids",
                                                             "device"}
        agent = cls(obs, act, agent_ids=ids, device=device, **{k: ck[k] for k in names if k in ck})
        agent.load_checkpoint(path)
        return agent

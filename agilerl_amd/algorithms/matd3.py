"""Drop-in ``MATD3`` (agilerl/algorithms/matd3.py:46-1060) for Box
observations and Discrete / Box actions, one network per agent: MADDPG
(algorithms/maddpg.py, whose networks, exploration noise, ``get_action``,
``test`` and architecture mutation it shares) with twin centralised critics
per agent and actor / target updates delayed by ``policy_freq``.

Of an update, the critic step of ``learn_individual`` — NaN rewards -> 0, NaN
dones -> 1, y = r + (1 - d) gamma min(Q1'(s', a'), Q2'(s', a')), MSE(Q1, y) +
MSE(Q2, y) and both gradients — is one libagx launch
(``agx_matd3_critic_target``).  On the GPU every optimizer step is one
``agx_clip_adam`` launch (no clip, as the reference does not clip) over the
network's flat parameter buffers (one ``FlatLearnState`` per agent and
group, flat_state.py), the torch optimizers staying the source of truth for
state_dict / checkpoints / clones, and the soft update of all 3 N networks is
one ``agx_polyak_segments`` launch over the 3 N flat (target, online) pairs.
On the CPU, or where a flat state does not apply, the torch optimizer steps
and the soft update goes tensor by tensor.

Outside this path (NotImplementedError): grouped (shared-policy) agents,
action masks and env-defined actions, custom actor / critic modules.
"""

from __future__ import annotations

from typing import Any

import torch

from .. import kernels as K
from . import checkpoint as C
from .evolvable import NetGroup
from .flat_state import flat_state
from .maddpg import _ACTORS, _MultiAgentPolicyGradient
from .offpolicy import MSECriticLoss


class MATD3(_MultiAgentPolicyGradient):
    algo = "MATD3"
    # matd3.py:444-461: lr_critic drives both sets of critic optimizers
    _groups = (_ACTORS, NetGroup("critics_1", "critic_targets_1", "critic_1_optimizers", "lr_critic"),
               NetGroup("critics_2", "critic_targets_2", "critic_2_optimizers", "lr_critic"))

    def __init__(self, observation_spaces, action_spaces, agent_ids: list[str] | None = None,
                 O_U_noise: bool = True, expl_noise: float = 0.1, vect_noise_dim: int = 1, mean_noise: float = 0.0,
                 theta: float = 0.15, dt: float = 1e-2, index: int = 0, hp_config=None, policy_freq: int = 2,
                 net_config: dict[str, Any] | None = None, batch_size: int = 64, lr_actor: float = 0.001,
                 lr_critic: float = 0.01, learn_step: int = 5, gamma: float = 0.95, tau: float = 0.01,
                 normalize_images: bool = True, mut=None, actor_networks=None, critic_networks=None, device="cuda",
                 accelerator=None, torch_compiler=None, wrap: bool = True) -> None:
        assert isinstance(wrap, bool), "Wrap models flag must be boolean value True or False."
        self._setup(observation_spaces, action_spaces, agent_ids, O_U_noise, expl_noise, vect_noise_dim, mean_noise,
                    theta, dt, index, hp_config, net_config, batch_size, lr_actor, lr_critic, learn_step, gamma, tau,
                    mut, (actor_networks, critic_networks), device, policy_freq=policy_freq)
        self.policy_freq = policy_freq
        self.learn_counter = dict.fromkeys(self.agent_ids, 0)

    def _construction_order(self) -> list[str]:
        """matd3.py:407-430: every group's networks, then every group's targets."""
        return [g.net for g in self._groups] + [g.target for g in self._groups]

    # ---- learning (matd3.py:700-926) --------------------------------------------
    def learn(self, experiences) -> dict[str, tuple[float | None, float]]:
        """One update from a sampled batch -> {agent id: (actor loss, or None
        when this call skipped the agent's actor, critic loss)}."""
        batch = self._batch(experiences)
        losses = {a: self.learn_individual(a, *batch) for a in self.agent_ids}
        if all(c % self.policy_freq == 0 for c in self.learn_counter.values()):
            self.soft_update_all()
        return losses

    def learn_individual(self, agent_id, stacked_actions, stacked_next_actions, states, next_states, actions,
                         rewards, dones) -> tuple[float | None, float]:
        critic_1, critic_2 = self.critics_1[agent_id], self.critics_2[agent_id]
        q_value_1 = critic_1(states, stacked_actions)
        q_value_2 = critic_2(states, stacked_actions)
        with torch.no_grad():
            q_next_1 = self.critic_targets_1[agent_id](next_states, stacked_next_actions)
            q_next_2 = self.critic_targets_2[agent_id](next_states, stacked_next_actions)
        # torch.min of the targets, NaN handling, y_j and both MSEs fused in
        # agx_matd3_critic_target (matd3.py:861-880)
        critic_loss = MSECriticLoss.apply(q_value_1, q_value_2, q_next_1, q_next_2,
                                          rewards[agent_id].float().reshape(-1), dones[agent_id].float().reshape(-1),
                                          float(self.gamma), True)
        self.critic_1_optimizers[agent_id].zero_grad()
        self.critic_2_optimizers[agent_id].zero_grad()
        critic_loss.backward()
        for g in self._groups[1:]:
            self._step(g, key=agent_id)

        # actor and targets every policy_freq learn steps.  The reference runs
        # the actor's forward on every call (matd3.py:898-900, before the
        # counter); a GumbelSoftmax output draws from torch's generator, so
        # the forward stays, without a graph when its result is not used
        self.learn_counter[agent_id] += 1
        delayed = self.learn_counter[agent_id] % self.policy_freq != 0
        with torch.set_grad_enabled(not delayed):
            action = self.actors[agent_id](states[agent_id])
        if delayed:
            return None, critic_loss.item()
        detached = {a: (action if a == agent_id else actions[a]) for a in self.agent_ids}
        actor_loss = -critic_1(states, torch.cat([detached[a] for a in self.agent_ids], dim=1)).mean()
        self.actor_optimizers[agent_id].zero_grad()
        actor_loss.backward()
        self._step(_ACTORS, key=agent_id)
        return actor_loss.item(), critic_loss.item()

    @torch.no_grad()
    def soft_update_all(self) -> None:
        """target <- tau * net + (1 - tau) * target for every network
        (matd3.py:770-782): one agx_polyak_segments launch over the flat
        (target, online) pairs; tensor by tensor (agx_polyak) for a network
        without a flat state."""
        targets, onlines = [], []
        for a in self.agent_ids:
            for g in self._groups:
                fs = flat_state(self, g, a)
                if fs is None:
                    self.soft_update(getattr(self, g.net)[a], getattr(self, g.target)[a])
                else:
                    targets.append(fs.tgt)
                    onlines.append(fs.prm)
        if targets:
            K.polyak_segments_(targets, onlines, float(self.tau))

    # ---- clones, checkpoints ------------------------------------------------------
    def clone(self, index: int | None = None, wrap: bool = True):
        """Deep copy with a new index (EvolvableAlgorithm.clone, core/base.py).
        The copy gets flat buffers of its own for every network whose flat
        state is live here, so its tensors are laid out as this agent's are
        and the two compute the same update from the same batch and seed."""
        flat = self.__dict__.pop("_flat", None) or {}
        try:
            c = super().clone(index, wrap)
        finally:
            if flat:
                self.__dict__["_flat"] = flat
        for g in self._groups:
            for a in self.agent_ids:
                fs = flat.get((g.net, a))
                if fs is not None and fs.valid(*(getattr(self, n)[a] for n in g[:3])):
                    flat_state(c, g, a)
        return c

    # core/base.py:939-1072 layout (checkpoint.py) with the reference's attribute names
    def _ckpt_extra(self, ck: dict) -> None:
        super()._ckpt_extra(ck)
        ck["policy_freq"], ck["learn_counter"] = int(self.policy_freq), C._plain(self.learn_counter)

    def _ckpt_restore(self, ck: dict) -> None:
        for k in ("lr_actor", "lr_critic", "policy_freq"):
            if k in ck:
                setattr(self, k, ck[k])
        if "learn_counter" in ck:
            self.learn_counter = {a: int(ck["learn_counter"].get(a, 0)) for a in self.agent_ids}

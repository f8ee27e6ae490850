"""The EvolvableAlgorithm hooks the reference's Mutations call
(agilerl/algorithms/core/base.py:744-775, hpo/mutation.py:413-453, 515-570)
for the object-level agents (DQN, RainbowDQN, DDPG, TD3, MADDPG, MATD3):

* ``registry``            the agent's HyperparameterConfig (hpo/registry.py);
* ``get_lr_names``        the attributes that are learning rates;
* ``reinit_optimizers``   a fresh Adam at the current learning rate — all of
                          them, or only the one whose lr was mutated
                          (mutation.py:440-450 ``to_reinit``);
* ``policy_weight_groups``the eval network's state dict(s) (one per agent id
                          for a ModuleDict policy, mutation.py:543-547), whose
                          2-D entries parameter mutations perturb in place;
* ``sync_shared_networks``the policy group's shared networks load the mutated
                          policy (mutation.py:554-561: the target networks);
* ``mutation_hook``       registered hooks (none for these algorithms)."""

from __future__ import annotations

import copy
from typing import NamedTuple

import torch

from .. import kernels as K
from ..modules.mlp import EvolvableMLP
from .flat_state import flat_state


class NetGroup(NamedTuple):
    """Attribute names of one eval network, its target copy, its optimizer and
    the learning rate that drives it (each a dict keyed by agent id in MADDPG / MATD3)."""
    net: str
    target: str
    opt: str
    lr: str


class EvolvableAgentMixin:
    sharded = False  # set by create_population when the agent is one shard of a global population

    #: the agent's networks; the first group is the policy group
    _groups: tuple[NetGroup, ...] = (NetGroup("actor", "actor_target", "optimizer", "lr"),)

    def _init_registry(self, hp_config) -> None:
        from ..hpo.registry import MutationRegistry

        self.hp_config = hp_config
        self.registry = MutationRegistry(hp_config)

    def get_lr_names(self) -> list[str]:
        return list(dict.fromkeys(g.lr for g in self._groups))

    def _triples(self) -> tuple[tuple[str, str, str], ...]:
        return tuple(g[:3] for g in self._groups)

    @property
    def can_mutate_architecture(self) -> bool:
        """MLP-encoder Q networks (the encoder's and head's node / layer
        mutations and the latent's); CNN encoders and multi-agent ModuleDicts
        are not mutated."""
        if getattr(self, "sharded", False):
            # a population sharded over ranks replays every global agent's draws
            # on every rank (hpo/shard.py RemoteAgent); the module and init draws
            # of a Q-network mutation are not replayed: not applied anywhere.
            # The flag is set by create_population and, for agents built any
            # other way, by the entry points' sharded mutation / selection
            # steps (hpo/shard.py mark_sharded): the off-policy loops treat
            # every multi-rank run as one population split over the ranks.
            return False
        from ..modules.cnn import EvolvableCNN

        net = getattr(self, self._groups[0].net)
        return isinstance(getattr(net, "encoder", None), (EvolvableMLP, EvolvableCNN)) and \
            isinstance(getattr(net, "head_net", None), EvolvableMLP)

    def architecture_mutation(self, new_layer_prob: float, rng) -> str:
        """mutation.py:829-885 on the policy network: the method sampled from
        its mutation table with ``rng`` (Mutations.rng; the table of an
        EvolvableNetwork with an MLP encoder, population/arch.py, or a CNN
        encoder, population/image_arch.py), applied
        with the modules' own generators; the shared (target) network re-made
        from the mutated one (reinit_shared_networks, mutation.py:104-160)."""
        net = getattr(self, self._groups[0].net)
        applied = net.apply_mutation(net.sample_mutation_method(new_layer_prob, rng))
        if self._groups[0].target:  # the bandits have no target copy
            setattr(self, self._groups[0].target, copy.deepcopy(net))
        return applied

    def reinit_optimizers(self, optimizer=None) -> None:
        """A fresh Adam at the current learning rate for every group, or for
        the groups that the learning rate named ``optimizer`` drives."""
        for g in self._groups:
            if optimizer in (None, g.lr):
                net, lr = getattr(self, g.net), getattr(self, g.lr)
                adam = lambda m: torch.optim.Adam(m.parameters(), lr=lr)  # noqa: E731
                setattr(self, g.opt, {a: adam(m) for a, m in net.items()} if hasattr(net, "items") else adam(net))

    def _step(self, group, max_norm: float = 0.0, key=None) -> None:
        """Where the reference calls ``optimizer.step()``: one launch over the
        group's flat buffers (flat_state.py), else the torch optimizer.
        ``key``: the agent id, for a group of dicts."""
        fs = flat_state(self, group) if key is None else flat_state(self, group, key)
        if fs is None or not fs.step(max_norm):
            opt = getattr(self, group[2])
            (opt if key is None else opt[key]).step()

    @torch.no_grad()
    def soft_update(self, group=None) -> None:
        """target <- tau * net + (1 - tau) * target: one agx_polyak launch over
        the group's flat buffers, else one per parameter tensor."""
        group = group or self._groups[0]
        fs = flat_state(self, group)
        if fs is not None:
            fs.polyak(self.tau)
        else:
            self._polyak_tensors(getattr(self, group[0]), getattr(self, group[1]))

    def _polyak_tensors(self, net, target) -> None:
        for n, t in ([(net[a], target[a]) for a in net] if hasattr(net, "items") else [(net, target)]):
            for e, p in zip(n.parameters(), t.parameters()):
                K.polyak_(p.data.view(-1), e.data.reshape(-1), float(self.tau))

    def clone(self, index: int | None = None, wrap: bool = True):
        """Deep copy with a new index (EvolvableAlgorithm.clone, core/base.py)."""
        c = copy.deepcopy(self)
        if index is not None:
            c.index = index
        return c

    def policy_weight_groups(self) -> list[dict[str, torch.Tensor]]:
        net = getattr(self, self._groups[0].net)
        if isinstance(net, torch.nn.ModuleDict):
            return [m.state_dict() for m in net.values()]
        return [net.state_dict()]

    @torch.no_grad()
    def sync_shared_networks(self) -> None:
        if not self._groups[0].target:
            return
        net, shared = (getattr(self, n) for n in self._groups[0][:2])
        if isinstance(net, torch.nn.ModuleDict):
            for k in net:
                shared[k].load_state_dict(net[k].state_dict(), strict=False)
        else:
            shared.load_state_dict(net.state_dict(), strict=False)

    def mutation_hook(self) -> None:
        pass

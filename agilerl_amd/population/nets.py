"""Population-stacked actor-critic MLPs over ONE flat parameter buffer [P, n].

Architecture (what the reference builds for PPO with a shared MLP encoder,
agilerl/utils/evolvable_networks.py:527-644 ``create_mlp`` via
agilerl/networks/base.py:541-561, ``StochasticActor`` / ``ValueNetwork``):

  encoder : [Linear -> LayerNorm(affine) -> act] per hidden size,
            Linear(-> latent) -> LayerNorm(no affine) -> act    (output_layernorm, output_vanish off)
  actor   : [Linear -> LayerNorm(affine) -> act] per hidden size, Linear(-> A)  (x0.1 init)
  critic  : same on the actor's latent (share_encoders, ppo.py:487-491), Linear(-> 1)

Every agent's parameters are one contiguous row of ``flat[P, n]`` laid out
[encoder | actor head | critic head] in state-dict order (weight, bias,
LN weight, LN bias per layer), so one kernel launch updates the whole
population and the two clip groups of ppo.py:910-911 are the contiguous
ranges [0, enc+actor) and [enc+actor, n).  Weights use the nn.Linear [out, in]
layout.  Initialisation: orthogonal (gain sqrt 2), zero bias, output layers
x0.1 (``layer_init`` / ``output_vanish``, evolvable_networks.py:410-441, 621-629).

``forward`` is the plain-PyTorch fp32 path (batched over the population with
bmm); it is the numerics reference for the fused HIP learner and the path
for architectures the fused kernel does not cover.
"""

from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F


@dataclass
class Layer:
    name: str
    fin: int
    fout: int
    ln: str | None  # None | "affine" | "plain"
    act: bool
    w: int = 0
    b: int = 0
    g: int = -1
    beta: int = -1
    vanish: bool = False


@dataclass
class ActorCriticSpec:
    obs_dim: int
    n_actions: int
    encoder_hidden: list[int] = field(default_factory=lambda: [64])
    latent_dim: int = 64
    actor_hidden: list[int] = field(default_factory=lambda: [64])
    critic_hidden: list[int] = field(default_factory=lambda: [64])
    layer_norm: bool = True
    # ppo.py:308: the actor's encoder is named "shared_encoder" when the critic
    # shares it (the reference default), so its layers are
    # shared_encoder_linear_layer_1, ... in the state dict
    encoder_name: str = "shared_encoder"
    # architecture-mutation limits (population/arch.py): per MLP (min / max
    # hidden layers, min / max nodes; EvolvableMLP's defaults 1, 3, 32, 500, or
    # MlpNetConfig's 1, 3, 16, 500) and the latent's (min, max)
    # (EvolvableNetwork: 8, 128)
    encoder_limits: tuple = (1, 3, 32, 500)
    actor_limits: tuple = (1, 3, 32, 500)
    critic_limits: tuple = (1, 3, 32, 500)
    latent_limits: tuple = (8, 128)
    # share_encoders=False (ppo.py:292-320): the critic has its own encoder
    # ("critic_encoder", the actor's is then "actor_encoder"), laid out after
    # the actor head in the reference's state-dict order
    share_encoders: bool = True
    critic_encoder_name: str = "critic_encoder"

    # the policy head over the actor's output: "categorical" (logits), or
    # "gaussian" (GaussianActorCriticSpec: the mean, with log_std parameters)
    head = "categorical"

    def shape_key(self) -> tuple:
        """Agents with equal keys share a network layout (population groups)."""
        return (self.obs_dim, self.n_actions, tuple(self.encoder_hidden), self.latent_dim, tuple(self.actor_hidden),
                tuple(self.critic_hidden), self.layer_norm, self.encoder_name, tuple(self.encoder_limits),
                tuple(self.actor_limits), tuple(self.critic_limits), tuple(self.latent_limits), self.share_encoders,
                self.critic_encoder_name)

    def __post_init__(self) -> None:
        ln = "affine" if self.layer_norm else None
        enc = [self.obs_dim, *self.encoder_hidden]
        def encoder(e):
            layers = [Layer(f"{e}_linear_layer_{i}", enc[i - 1], enc[i], ln, True) for i in range(1, len(enc))]
            layers.append(Layer(f"{e}_linear_layer_output", enc[-1], self.latent_dim,
                                "plain" if self.layer_norm else None, True))
            return layers

        self.encoder = encoder(self.encoder_name)
        self.critic_encoder = [] if self.share_encoders else encoder(self.critic_encoder_name)
        self.actor = self._head("actor", self.actor_hidden, self.n_actions, ln)
        self.critic = self._head("value", self.critic_hidden, 1, ln)  # ValueNetwork head name (value_networks.py:96)
        off = 0
        for lay in self.encoder + self.actor + self.critic_encoder + self.critic:
            lay.w = off
            off += lay.fin * lay.fout
            lay.b = off
            off += lay.fout
            if lay.ln == "affine":
                lay.g = off
                off += lay.fout
                lay.beta = off
                off += lay.fout
            if lay is self.actor[-1]:
                off = self._after_actor_output(off)
                self.actor_end = off
        self.n_params = off
        self.group_offsets = [0, self.actor_end, self.n_params]

    def _after_actor_output(self, off: int) -> int:
        """Parameters of the policy head that no layer owns, laid out at
        ``off`` (the end of the actor's output layer) -> the actor group's end."""
        return off

    def _head(self, name, hidden, nout, ln):
        dims = [self.latent_dim, *hidden]
        layers = [Layer(f"{name}_linear_layer_{i}", dims[i - 1], dims[i], ln, True)
                  for i in range(1, len(dims))]
        layers.append(Layer(f"{name}_linear_layer_output", dims[-1], nout, None, False, vanish=True))
        return layers

    @property
    def layers(self) -> list[Layer]:
        return self.encoder + self.actor + self.critic_encoder + self.critic

    def aliased(self, key: str) -> bool:
        """A state-dict key whose tensor is another key's (the shared
        encoder's critic copy)."""
        return self.share_encoders and key.startswith("critic.encoder.")

    # ------------------------------------------------------------------ #
    def init_params(self, P: int, seeds: list[int] | None = None, device="cpu") -> torch.Tensor:
        flat = torch.zeros(P, self.n_params, dtype=torch.float32)
        for p in range(P):
            gen = torch.Generator().manual_seed(int(seeds[p]) if seeds is not None else p)
            for lay in self.layers:
                w = torch.empty(lay.fout, lay.fin)
                torch.nn.init.orthogonal_(w, math.sqrt(2), generator=gen)
                if lay.vanish:
                    w.mul_(0.1)
                flat[p, lay.w: lay.w + w.numel()] = w.reshape(-1)
                if lay.ln == "affine":
                    flat[p, lay.g: lay.g + lay.fout] = 1.0
        return flat.to(device)

    def views(self, flat: torch.Tensor, lay: Layer):
        P = flat.shape[0]
        W = flat[:, lay.w: lay.w + lay.fin * lay.fout].view(P, lay.fout, lay.fin)
        b = flat[:, lay.b: lay.b + lay.fout]
        g = flat[:, lay.g: lay.g + lay.fout] if lay.ln == "affine" else None
        be = flat[:, lay.beta: lay.beta + lay.fout] if lay.ln == "affine" else None
        return W, b, g, be

    def _run(self, flat, x, layers):
        """Agent by agent: 2-D GEMMs whose kernel choice (and so rounding)
        depends only on the agent's own shapes, never on how many agents the
        population holds — a population split into groups or sharded over
        ranks computes exactly what the whole one does."""
        outs = []
        for p in range(flat.shape[0]):
            h = x[p]
            for lay in layers:
                W, b, g, be = self.views(flat[p:p + 1], lay)
                h = torch.addmm(b[0], h, W[0].t())
                if lay.ln is not None:
                    h = F.layer_norm(h, (lay.fout,), eps=1e-5)
                    if g is not None:
                        h = h * g[0] + be[0]
                if lay.act:
                    h = torch.relu(h)
            outs.append(h)
        return torch.stack(outs)

    def forward(self, flat: torch.Tensor, obs: torch.Tensor):
        """obs [P, B, obs_dim] -> (logits [P, B, A], value [P, B])."""
        lat = self._run(flat, obs, self.encoder)
        logits = self._run(flat, lat, self.actor)
        lat_c = lat if self.share_encoders else self._run(flat, obs, self.critic_encoder)
        value = self._run(flat, lat_c, self.critic).squeeze(-1)
        return logits, value

    def state_dict_keys(self) -> dict[str, tuple[int, tuple[int, ...]]]:
        """Reference-compatible parameter names -> (offset, shape)."""
        out = {}
        # critic.encoder is the reference's detached copy of the shared actor encoder
        # (share_encoders, algo_utils.py:164-187): same offsets as actor.encoder
        # the actor's head is an EvolvableDistribution wrapping the MLP
        # (networks/actors.py:330-336, modules/base.py:740-760): its
        # parameters sit under head_net._wrapped in the reference's state dict
        for net, layers in (("actor.encoder.model", self.encoder), ("actor.head_net._wrapped.model", self.actor),
                            ("critic.encoder.model", self.encoder if self.share_encoders else self.critic_encoder),
                            ("critic.head_net.model", self.critic)):
            for lay in layers:
                out[f"{net}.{lay.name}.weight"] = (lay.w, (lay.fout, lay.fin))
                out[f"{net}.{lay.name}.bias"] = (lay.b, (lay.fout,))
                if lay.ln == "affine":
                    ln_name = lay.name.replace("linear_layer", "layer_norm")
                    out[f"{net}.{ln_name}.weight"] = (lay.g, (lay.fout,))
                    out[f"{net}.{ln_name}.bias"] = (lay.beta, (lay.fout,))
        return out

    def _head_descriptor(self, check):
        """The layer list when ``check(lib, head, descriptor)`` (pure host-side
        validation) admits it; None otherwise, or for the categorical head."""
        import ctypes

        from .. import _lib
        from .learner import layer_list
        from .ppo_pop import HEADS

        head = HEADS.get(self.head)
        d = layer_list(self) if head is not None else None
        if d is None or not check(_lib.load(require_gpu=False), head, ctypes.byref(d)):
            return None
        return d

    def act_descriptor(self):
        """agx_ppo_graph of a non-categorical head's networks (ppo_pop.HEADS) for
        agx_ppo_act_<stem>_graph (a Gaussian spec's n_params counts the log_std
        floats, which no layer owns), or None when the layer list is outside
        what the kernel takes."""
        return self._head_descriptor(
            lambda lib, h, d: getattr(lib, f"agx_ppo_act_{h.stem}_graph_workspace_bytes")(d, 1, 1) != 0)

    def learn_descriptor_head(self):
        """agx_ppo_graph of such networks for agx_ppo_learn_<stem>_graph (the
        head's own arguments after it: ``log_std``, ``multi_head()``, nothing),
        or None when that learner does not take the layer list: then the
        autograd learner runs."""
        return self._head_descriptor(
            lambda lib, h, d: getattr(lib, f"agx_ppo_{h.stem}_graph_check")(d, *h.lead(self)) == 0)


@dataclass
class GaussianActorCriticSpec(ActorCriticSpec):
    """The actor-critic of a Box action space (networks/actors.py:296-336 with
    networks/distributions.py:152-183): the actor's output layer gives the mean
    of a diagonal Gaussian, and the distribution wrapper's ``log_std`` [1, A]
    (filled with ``action_std_init``) is a parameter of the actor.  The A
    log_std floats sit directly after the actor's output layer, inside the
    actor clip group [0, actor_end) (ppo.py:910-911).  ``n_actions`` is the
    action dimension A.  The categorical kernels (agx_ppo_learn, agx_ppo_act,
    the persistent rollout and evaluation) never see this spec: the Gaussian
    policy step is agx_ppo_act_gauss_graph over ``act_descriptor()``."""

    action_std_init: float = 0.0
    log_std: int = -1  # offset of the A log_std floats in the row (set by __post_init__)
    # the Box's bounds (A floats each, inf where unbounded): what the env's copy
    # of an action is clipped to at inference (ppo.py:604-614); () = unbounded
    action_low: tuple = ()
    action_high: tuple = ()

    head = "gaussian"

    @property
    def action_dim(self) -> int:
        return self.n_actions

    def shape_key(self) -> tuple:
        return super().shape_key() + (self.head, float(self.action_std_init), tuple(self.action_low),
                                      tuple(self.action_high))

    def _after_actor_output(self, off: int) -> int:
        self.log_std = off
        return off + self.n_actions

    def init_params(self, P: int, seeds: list[int] | None = None, device="cpu") -> torch.Tensor:
        flat = super().init_params(P, seeds, "cpu")  # the layers draw exactly as a Discrete spec's
        flat[:, self.log_std: self.log_std + self.n_actions] = float(self.action_std_init)
        return flat.to(device)

    def log_std_view(self, flat: torch.Tensor) -> torch.Tensor:
        """[P, A] view of the agents' log_std."""
        return flat[:, self.log_std: self.log_std + self.n_actions]

    gauss_descriptor = ActorCriticSpec.act_descriptor  # the names the head came with
    gauss_learn_descriptor = ActorCriticSpec.learn_descriptor_head

    def state_dict_keys(self) -> dict[str, tuple[int, tuple[int, ...]]]:
        # log_std is the distribution wrapper's own parameter, so it precedes
        # head_net._wrapped.* in the reference's actor.parameters() / state dict
        # (distributions.py:152-156); the flat row has it after the output layer
        out = {}
        for k, v in super().state_dict_keys().items():
            if "actor.head_net.log_std" not in out and k.startswith("actor.head_net._wrapped."):
                out["actor.head_net.log_std"] = (self.log_std, (1, self.n_actions))
            out[k] = v
        return out


@dataclass
class MultiDiscreteActorCriticSpec(ActorCriticSpec):
    """The actor-critic of a MultiDiscrete action space (networks/actors.py:268
    with networks/distributions.py:193-199): one categorical per component over
    slices of the actor's L = sum(nvec) logits.  ``n_actions`` is L, so the
    layer list, the parameter order and the initial draws are those of the
    categorical spec with n = L; there are no extra parameters.  The categorical
    kernels (agx_ppo_learn, agx_ppo_learn_graph, agx_ppo_act, the persistent
    rollout and evaluation) never see this spec, K = 1 included: the policy
    step is agx_ppo_act_multi_graph over ``act_descriptor()`` and the fused
    learner agx_ppo_learn_multi_graph over ``learn_descriptor_head()``."""

    nvec: tuple = ()

    head = "multidiscrete"

    def __post_init__(self) -> None:
        self.nvec = tuple(int(n) for n in self.nvec)
        if not self.nvec or min(self.nvec) < 1 or sum(self.nvec) != self.n_actions:
            raise ValueError(f"nvec {self.nvec} must hold K >= 1 positive sizes that sum to n_actions "
                             f"({self.n_actions})")
        super().__post_init__()

    @property
    def n_components(self) -> int:
        return len(self.nvec)

    def shape_key(self) -> tuple:
        return super().shape_key() + (self.head, self.nvec)

    def multi_head(self):
        """agx_multi_head (include/agx_multi.h) of nvec, passed by value."""
        from ..kernels import multi_head

        return multi_head(self.nvec)

    multi_descriptor = ActorCriticSpec.act_descriptor  # the names the head came with
    multi_learn_descriptor = ActorCriticSpec.learn_descriptor_head


@dataclass
class MultiBinaryActorCriticSpec(ActorCriticSpec):
    """The actor-critic of a MultiBinary action space (networks/actors.py:268
    with networks/distributions.py:201-207): one independent Bernoulli per
    logit of the actor's n outputs.  ``n_actions`` is n, so the layer list, the
    parameter order and the initial draws are those of the categorical spec
    with n actions; there are no extra parameters.  The categorical kernels
    never see this spec: the policy step is agx_ppo_act_bern_graph over
    ``act_descriptor()`` and the fused learner agx_ppo_learn_bern_graph over
    ``learn_descriptor_head()``.  ``action_dtype``: the space's numpy dtype
    name, what the env is handed its 0 / 1 actions in."""

    action_dtype: str = "int8"

    head = "multibinary"

    def __post_init__(self) -> None:
        if not 1 <= int(self.n_actions) <= 32:
            raise ValueError(f"a MultiBinary head takes 1..32 bits (got {self.n_actions})")
        super().__post_init__()

    @property
    def n_components(self) -> int:
        return self.n_actions

    def shape_key(self) -> tuple:
        return super().shape_key() + (self.head, self.action_dtype)

    bern_descriptor = ActorCriticSpec.act_descriptor  # the names the head came with
    bern_learn_descriptor = ActorCriticSpec.learn_descriptor_head


def bernoulli_head(logits: torch.Tensor, action: torch.Tensor, mask: torch.Tensor | None = None):
    """log-prob of ``action`` [..., n] (anything but 0 counts as 1) and entropy
    of n independent Bernoullis over ``logits`` [..., n] as
    ``agilerl/utils/torch_utils.py:348-376`` (illegal logits -> -1e8 first,
    distributions.py:16-28), in the form of include/agx_bernoulli.h: finite
    for |logit| up to 1e8.  -> (logp [...], entropy [...])."""
    if mask is not None:
        logits = torch.where(mask.bool(), logits, torch.full_like(logits, -1e8))
    s = torch.log1p(torch.exp(-logits.abs()))
    log_p = torch.clamp(logits, max=0.0) - s
    log_q = torch.clamp(-logits, max=0.0) - s
    logp = torch.where(action != 0, log_p, log_q).sum(-1)
    p, q = torch.sigmoid(logits), torch.sigmoid(-logits)
    ent = -(p * torch.log(p + 1e-8) + q * torch.log(q + 1e-8)).sum(-1)
    return logp, ent


def multi_categorical(logits: torch.Tensor, nvec, action: torch.Tensor, mask: torch.Tensor | None = None):
    """log-prob of ``action`` [..., K] and entropy of the K categoricals over
    slices of ``logits`` [..., L] as ``agilerl/utils/torch_utils.py:284-333``
    (illegal logits -> -1e8 first, distributions.py:16-28); both summed over
    the components in ascending order.  -> (logp [...], entropy [...])."""
    if mask is not None:
        logits = torch.where(mask.bool(), logits, torch.full_like(logits, -1e8))
    logp = ent = None
    off = 0
    for k, n in enumerate(nvec):
        logp_all, h = categorical(logits[..., off:off + n])
        lp = logp_all.gather(-1, action[..., k:k + 1]).squeeze(-1)
        logp = lp if logp is None else logp + lp
        ent = h if ent is None else ent + h
        off += n
    return logp, ent


def categorical(logits: torch.Tensor):
    """log-softmax and entropy as ``agilerl/utils/torch_utils.py:142-199``:
    H = -sum p * log(p + 1e-8)."""
    logp_all = torch.log_softmax(logits, dim=-1)
    p = torch.softmax(logits, dim=-1)
    ent = -(p * torch.log(p + 1e-8)).sum(-1)
    return logp_all, ent


_LOG_2PI = math.log(2 * math.pi)


def gaussian(mean: torch.Tensor, log_std: torch.Tensor, action: torch.Tensor):
    """log-prob of ``action`` and entropy of the diagonal Gaussian N(mean,
    exp(log_std)^2) as ``agilerl/utils/torch_utils.py:225-257``; log_std
    broadcasts against mean [..., A].  -> (logp [...], entropy [...])."""
    log_std = log_std.expand_as(mean)
    var = torch.exp(2 * log_std)
    logp = (-0.5 * ((action - mean) ** 2 / var + 2 * log_std + _LOG_2PI)).sum(-1)
    ent = 0.5 * (1 + _LOG_2PI) * mean.size(-1) + log_std.sum(-1)
    return logp, ent

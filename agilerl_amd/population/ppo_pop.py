"""A PPO population resident in HBM: stacked networks, SoA rollout storage,
batched rollout inference and a batched learner.

Reference behaviour mirrored per agent:
  * rollout collection  agilerl/rollouts/on_policy.py:23-203 (done = term|trunc
    of THIS step; bootstrap with last_done = term, :184-196)
  * rollout storage     agilerl/components/rollout_buffer.py:137-411 (time-major
    (T, N) SoA; here (P, T, N) on the GPU instead of CPU TensorDicts)
  * GAE                 rollout_buffer.py:413-481 -> agx_gae (bit-exact)
  * learner             agilerl/algorithms/ppo.py:814-921: global advantage
    normalisation, E epochs of shuffled minibatches, clipped surrogate +
    clipped value loss - entropy, per-group grad clip, Adam;
    returns sum(loss)/(num_samples*epochs) (:920)

The population axis replaces the reference's sequential agent loop
(train_on_policy.py:210): every kernel processes all P agents at once.
Sampling uses an on-device Gumbel-max draw (the reference's torch.multinomial
stream cannot be reproduced on a GPU generator anyway).  Minibatch order is
the reference's: by default the permutations come from numpy's global
legacy MT19937 exactly as PPO.learn's ``np.random.shuffle`` draws them
(``perm_source="numpy"``, agilerl_amd/rng.py); ``perm_source="device"``
draws them on the GPU instead (no host work, not reproducible against the
reference).

Two learner back ends share this state:
  * ``fused=True``  one persistent HIP workgroup per agent runs all E x M
                    minibatch updates (agx_ppo_learn, f32 MFMA GEMMs) —
                    the production path;
  * ``fused=False`` plain-PyTorch fp32 autograd over the stacked networks with
                    the HIP loss / clip+Adam kernels — the numerics reference
                    for the fused kernel and the path for architectures it does
                    not cover.

A Gaussian spec (Box actions, nets.GaussianActorCriticSpec) stores float
actions (P, T, N, A), acts through agx_ppo_act_gauss_graph and learns through
agx_ppo_learn_gauss_graph (the runtime-shape learner with a Gaussian head);
with ``fused=False``, AGX_GAUSS_FUSED=0 or a layer list that learner does not
take, on the autograd path with the fused Gaussian loss kernel
(agx_ppo_gauss_loss_fwd_bwd).  The categorical kernels never see it.

A MultiDiscrete spec (nets.MultiDiscreteActorCriticSpec) stores int64 actions
(P, T, N, K) and flat masks (P, T, N, L) and acts through
agx_ppo_act_multi_graph; the categorical kernels never see it either, K = 1
included.  By default it learns on the autograd path with the fused
multi-categorical loss kernel (agx_ppo_multi_loss_fwd_bwd).  Built with
``multi_fused=True``, or with AGX_MULTI_FUSED=1 in the environment, it learns
through agx_ppo_learn_multi_graph (the runtime-shape learner with a
multi-categorical head) instead; ``fused=False`` or a layer list that learner
does not take keeps the autograd path whatever the switch says.  The switch is
opt-in for now: the default build of such a population behaves as before.

A MultiBinary spec (nets.MultiBinaryActorCriticSpec) reuses that storage with
one column per bit: int64 actions (P, T, N, n) holding 0 / 1 and flat masks
(P, T, N, n).  It acts through agx_ppo_act_bern_graph and learns through
agx_ppo_learn_bern_graph (the runtime-shape learner with a Bernoulli head);
with ``fused=False``, AGX_BERN_FUSED=0 or a layer list that learner does not
take, on the autograd path with the fused Bernoulli loss kernel
(agx_ppo_bern_loss_fwd_bwd).  ``vector_int`` is true of both kinds of
population, ``act_width`` their action columns (K or n).
"""

from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib
from .. import kernels as K
from .nets import ActorCriticSpec, categorical
from .perms import MinibatchOrders


class _PPOLossFn(torch.autograd.Function):
    """Clipped surrogate loss for P minibatches at once (HIP fwd+bwd)."""

    @staticmethod
    def forward(ctx, logp, value, entropy, old_logp, adv, ret, old_v, gidx, b, clip, vf, ent):
        g1, g2, g3, stats = K.ppo_loss_fwd_bwd(
            logp.contiguous().view(-1), old_logp, adv, ret, old_v, value.contiguous().view(-1),
            entropy.contiguous().view(-1), b, clip, vf, ent, index=gidx)
        ctx.save_for_backward(g1, g2, g3)
        ctx.shape = logp.shape
        ctx.mark_non_differentiable(stats)
        return stats[:, 0].sum(), stats

    @staticmethod
    def backward(ctx, gl, _gs):
        g1, g2, g3 = ctx.saved_tensors
        s = ctx.shape
        return (g1.view(s) * gl, g2.view(s) * gl, g3.view(s) * gl) + (None,) * 9


class _PPOGaussLossFn(torch.autograd.Function):
    """_PPOLossFn for a Gaussian head (agx_ppo_gauss_loss_fwd_bwd): the
    log-prob of the stored actions, the entropy and the loss in one launch;
    ``log_std`` [P, A] is the slice of the parameter rows, so its gradient
    lands in the rows' gradient through autograd's slice backward."""

    @staticmethod
    def forward(ctx, mean, value, log_std, actions, old_logp, adv, ret, old_v, gidx, b, clip, vf, ent):
        A = mean.shape[-1]
        g1, g2, g3, stats = K.ppo_gauss_loss_fwd_bwd(
            mean.contiguous().view(-1, A), value.contiguous().view(-1), log_std.contiguous(), actions, old_logp,
            adv, ret, old_v, b, clip, vf, ent, index=gidx)
        ctx.save_for_backward(g1, g2, g3)
        ctx.shapes = (mean.shape, value.shape, log_std.shape)
        ctx.mark_non_differentiable(stats)
        return stats[:, 0].sum(), stats

    @staticmethod
    def backward(ctx, gl, _gs):
        g1, g2, g3 = ctx.saved_tensors
        sm, sv, sl = ctx.shapes
        return (g1.view(sm) * gl, g2.view(sv) * gl, g3.view(sl) * gl) + (None,) * 10


class _PPOMultiLossFn(torch.autograd.Function):
    """_PPOLossFn for a multi-categorical head (agx_ppo_multi_loss_fwd_bwd):
    the masked per-component log-softmax, the log-prob of the stored actions
    [rows, K], the entropy and the loss in one launch; ``logits`` are the raw
    network output, and a masked logit gets gradient 0."""

    @staticmethod
    def forward(ctx, logits, value, head, actions, masks, old_logp, adv, ret, old_v, gidx, b, clip, vf, ent):
        L = logits.shape[-1]
        g1, g2, stats = K.ppo_multi_loss_fwd_bwd(
            logits.contiguous().view(-1, L), value.contiguous().view(-1), head, actions, old_logp, adv, ret, old_v,
            b, clip, vf, ent, index=gidx, mask=masks)
        ctx.save_for_backward(g1, g2)
        ctx.shapes = (logits.shape, value.shape)
        ctx.mark_non_differentiable(stats)
        return stats[:, 0].sum(), stats

    @staticmethod
    def backward(ctx, gl, _gs):
        g1, g2 = ctx.saved_tensors
        sl, sv = ctx.shapes
        return (g1.view(sl) * gl, g2.view(sv) * gl) + (None,) * 12


class _PPOBernLossFn(torch.autograd.Function):
    """_PPOLossFn for a Bernoulli head (agx_ppo_bern_loss_fwd_bwd): the masked
    logits, the log-prob of the stored bits [rows, n], the entropy and the loss
    in one launch; ``logits`` are the raw network output, and a masked logit
    gets gradient 0."""

    @staticmethod
    def forward(ctx, logits, value, actions, masks, old_logp, adv, ret, old_v, gidx, b, clip, vf, ent):
        n = logits.shape[-1]
        g1, g2, stats = K.ppo_bern_loss_fwd_bwd(
            logits.contiguous().view(-1, n), value.contiguous().view(-1), actions, old_logp, adv, ret, old_v,
            b, clip, vf, ent, index=gidx, mask=masks)
        ctx.save_for_backward(g1, g2)
        ctx.shapes = (logits.shape, value.shape)
        ctx.mark_non_differentiable(stats)
        return stats[:, 0].sum(), stats

    @staticmethod
    def backward(ctx, gl, _gs):
        g1, g2 = ctx.saved_tensors
        sl, sv = ctx.shapes
        return (g1.view(sl) * gl, g2.view(sv) * gl) + (None,) * 11


@dataclass
class Head:
    """What the host side needs to know of a non-categorical action head; the
    entry points are agx_ppo_act_<stem>_graph, agx_ppo_rollout_<stem>_graph_
    persistent, agx_ppo_eval_<stem>_graph_persistent, agx_ppo_<stem>_graph_check
    and agx_ppo_learn_<stem>_graph, each taking ``lead(spec)`` right after the
    network descriptor."""

    stem: str
    lead: object          # spec -> the arguments after the descriptor
    dtype: torch.dtype    # a stored action's element
    width: object         # spec -> action columns per row
    clip: bool            # the launches take (clip_low, clip_high) for the env's copy
    masks: bool           # the per-step launch takes a legal-action mask
    fused_env: str        # the fused learner's environment switch ...
    fused_default: bool   # ... what holds while it is unset (only "0" / "1" flips it) ...
    multi_fused: bool     # ... and whether the ``multi_fused`` keyword switches it on too

    def __post_init__(self) -> None:
        self.act = f"agx_ppo_act_{self.stem}_graph"  # the per-step entry point (the name each step looks up)

    def fused_on(self, pop) -> bool:
        flipped = os.environ.get(self.fused_env) == ("0" if self.fused_default else "1")
        return (self.fused_default != flipped) or (self.multi_fused and pop.multi_fused)


HEADS = {  # keyed by spec.head
    "gaussian": Head("gauss", lambda s: (s.log_std,), torch.float32, lambda s: s.n_actions, True, False,
                     "AGX_GAUSS_FUSED", True, False),
    "multidiscrete": Head("multi", lambda s: (s.multi_head(),), torch.int64, lambda s: len(s.nvec), False, True,
                          "AGX_MULTI_FUSED", False, True),
    "multibinary": Head("bern", lambda s: (), torch.int64, lambda s: s.n_actions, False, True,
                        "AGX_BERN_FUSED", True, False),
}


class PPOPopulation:
    # a non-categorical population's descriptors and head arguments, made on first use
    _hdesc = None
    _hlearn = None
    _mhead = None

    @property
    def head(self) -> Head | None:
        """The population's entry of HEADS; None: the categorical head."""
        return HEADS.get(getattr(self.spec, "head", "categorical"))

    @property
    def multibinary(self) -> bool:
        """A MultiBinary action space: the MultiDiscrete storage with one column
        per bit (0 / 1), the Bernoulli policy step, loss and learner
        (agx_bernoulli.h)."""
        return getattr(self.spec, "head", "categorical") == "multibinary"

    @property
    def vector_int(self) -> bool:
        """int64 action vectors [.., act_width]: MultiDiscrete or MultiBinary."""
        return self.multidiscrete or self.multibinary

    @property
    def act_width(self) -> int:
        """Stored action columns per row: A dimensions, K components, n bits, else 1."""
        return 1 if self.head is None else self.head.width(self.spec)

    def __init__(self, spec: ActorCriticSpec, pop_size: int, num_envs: int, *, learn_step=2048,
                 batch_size=128, lr=1e-3, gamma=0.99, gae_lambda=0.95, clip_coef=0.2, ent_coef=0.01,
                 vf_coef=0.5, max_grad_norm=0.5, update_epochs=4, target_kl=None, seeds=None,
                 device="cuda", fused=True, perm_source="numpy", action_masks=False, agent_offset=0,
                 global_pop_size=None, seed_base=None, agent_ids=None, init_params=True, multi_fused=False):
        self.spec = spec
        # a Box action space: float actions [.., A], the Gaussian policy step and loss (agx_gauss.h)
        self.gaussian = getattr(spec, "head", "categorical") == "gaussian"
        if self.gaussian and action_masks:
            raise ValueError("action masks apply to Discrete action spaces, not to a Gaussian policy")
        # a MultiDiscrete action space: int64 actions [.., K], flat masks [.., L], the
        # multi-categorical policy step and loss (agx_multi.h); K = 1 included
        self.multidiscrete = getattr(spec, "head", "categorical") == "multidiscrete"
        self.P, self.N = int(pop_size), int(num_envs)
        # a shard of a population spread over ranks: these P agents are global
        # agents agent_offset .. agent_offset + P of global_pop_size (their
        # sampling streams, env copies and minibatch shuffles are the global
        # agents' own, so the sharded run draws what one process would)
        self.agent_offset = int(agent_offset)
        self.global_P = self.P if global_pop_size is None else int(global_pop_size)
        if self.agent_offset < 0 or self.agent_offset + self.P > self.global_P:
            raise ValueError("agent_offset / global_pop_size do not contain this shard")
        # global index of each local agent (a contiguous shard by default; a
        # group of the population engine holds any subset): keys its env
        # copies' sampling streams
        self.agent_ids = (list(range(self.agent_offset, self.agent_offset + self.P)) if agent_ids is None
                          else [int(i) for i in agent_ids])
        if len(self.agent_ids) != self.P:
            raise ValueError("agent_ids must name every agent")
        self.T = -(learn_step // -self.N)  # capacity = ceil(learn_step / num_envs), ppo.py:363
        self.S = self.T * self.N
        self.batch_size = int(batch_size)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.clip_coef, self.ent_coef, self.vf_coef = float(clip_coef), float(ent_coef), float(vf_coef)
        self.max_grad_norm = float(max_grad_norm)
        self.update_epochs = int(update_epochs)
        self.target_kl = target_kl
        self.device = torch.device(device)
        seeds = list(range(self.agent_offset, self.agent_offset + self.P)) if seeds is None else list(seeds)
        self.seeds = seeds
        # population-level streams key off the global population's first seed
        seed_base = int(seeds[0]) if seed_base is None else int(seed_base)
        self.seed_base = seed_base
        # init_params=False: zeros, for a caller that copies every row in (the
        # population engine's regrouping; the orthogonal init is a host QR per layer)
        self.params = torch.nn.Parameter(spec.init_params(self.P, seeds, self.device) if init_params else
                                         torch.zeros(self.P, spec.n_params, dtype=torch.float32, device=self.device))
        self.params.grad = torch.zeros_like(self.params)
        lr_list = [float(lr)] * self.P if not isinstance(lr, (list, tuple)) else [float(x) for x in lr]
        self.opt = K.ClipAdam(self.params.data, spec.group_offsets, lr_list, max_norm=self.max_grad_norm,
                              grads=self.params.grad)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed_base * 7919 + 17)
        if perm_source not in ("numpy", "device"):
            raise ValueError("perm_source must be 'numpy' or 'device'")
        self.perm_source = perm_source
        self.use_action_masks = bool(action_masks)
        # sticky device error word of the fused learner (partner timeout); checked at host sync points
        self.err_word = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.last_kl = None
        # per-agent RL hyperparameters (mutation.py:413-453 mutates them agent by
        # agent); batch_size / update_epochs above are the population maxima
        self.agent_batch = [self.batch_size] * self.P
        self.agent_epochs = [self.update_epochs] * self.P
        self.agent_ent = [self.ent_coef] * self.P
        self.agent_lr = list(lr_list)  # exact host values (the device table is f32)
        # device copies (the learner reads them once the population is heterogeneous;
        # PopulationSync moves them with the parent rows)
        self.hp_batch_d = torch.full((self.P,), self.batch_size, dtype=torch.int32, device=self.device)
        self.hp_epochs_d = torch.full((self.P,), self.update_epochs, dtype=torch.int32, device=self.device)
        self.hp_ent_d = torch.full((self.P,), self.ent_coef, dtype=torch.float32, device=self.device)
        self._hetero = False
        self.fused = fused
        # a MultiDiscrete population learns on agx_ppo_learn_multi_graph only when asked to
        # (this keyword, or AGX_MULTI_FUSED=1 when the descriptor is first wanted)
        self.multi_fused = bool(multi_fused)
        self.act_seed = (seed_base * 0x9E3779B97F4A7C15 + 0x5851F42D) & 0xFFFFFFFFFFFFFFFF
        # every global agent's update_epochs (the shuffles each draws; ranks
        # refresh the other shards' entries after a mutation)
        self.global_epochs = [self.update_epochs] * self.global_P
        self.global_batch_max = None
        self.act_counter = 0
        self._desc = None
        self._gdesc = None
        self._edesc = None
        self._alloc_rollout()
        self.env_base_d = torch.tensor([i * self.N for i in self.agent_ids], dtype=torch.int64, device=self.device)
        self.learn_steps = 0
        self.rollout_id = 0
        self.prefetch_perms = os.environ.get("AGX_PREFETCH_PERMS", "1") != "0"
        self.orders = MinibatchOrders(self)  # which permutation the next learn() gets (perms.py)
        self._gae_launch = None

    # ------------------------------------------------------------------ #
    def _alloc_rollout(self):
        P, T, N, D, dev = self.P, self.T, self.N, self.spec.obs_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # image specs keep uint8 frames (normalised inside the first conv's load)
        self.obs = torch.zeros(P, T, N, D, dtype=getattr(self.spec, "obs_dtype", torch.float32), device=dev)
        self.actions = (torch.zeros(P, T, N, self.spec.n_actions, dtype=torch.float32, device=dev) if self.gaussian
                        else torch.zeros(P, T, N, self.act_width, dtype=torch.int64, device=dev)
                        if self.vector_int else torch.zeros(P, T, N, dtype=torch.int64, device=dev))
        self.rewards = torch.zeros(P, T, N, **f32)
        self.dones = torch.zeros(P, T, N, dtype=torch.uint8, device=dev)
        self.values = torch.zeros(P, T, N, **f32)
        self.log_probs = torch.zeros(P, T, N, **f32)
        self.advantages = torch.zeros(P, T, N, **f32)
        self.returns = torch.zeros(P, T, N, **f32)
        self.adv_stats = torch.zeros(P, 2, dtype=torch.float64, device=dev)
        # legal-action masks (1 = legal) stored with the rollout when the env provides them
        self.action_masks = (torch.ones(P, T, N, self.spec.n_actions, dtype=torch.uint8, device=dev)
                             if self.use_action_masks else None)
        self.gae_ws = torch.empty(max(16, K._lib.load().agx_gae_workspace_bytes(P, T, N)), dtype=torch.uint8,
                                  device=dev)

    # ------------------------------------------------------------------ #
    @torch.no_grad()
    def act(self, obs: torch.Tensor, counter: int | None = None):
        """obs [P, N, D] (device) -> action, log_prob, entropy, value, each [P, N].
        Gumbel-max sampling; with ``counter`` every agent draws from its own
        generator keyed by (population seed, global agent id, counter), so an
        agent's draws do not depend on which other agents share its population.
        A Gaussian population: one agx_ppo_act_gauss_graph launch, float
        actions [P, N, A] (``counter`` None: the next rollout counter)."""
        if self.head is not None:  # one agx_ppo_act_<stem>_graph launch, actions [P, N, act_width]
            if counter is None:
                self.act_counter += 1
                counter = self.act_counter
            return self._head_step(obs, sample=True, counter=int(counter))
        logits, value = self.spec.forward(self.params.data, obs)
        logp_all, ent = categorical(logits)
        if counter is None:
            u = torch.rand(logits.shape, generator=self.gen, device=self.device)
        else:
            u = torch.empty(logits.shape, device=self.device)
            g = torch.Generator(device=self.device)
            for p, aid in enumerate(self.agent_ids):
                g.manual_seed(((self.seed_base * 1_000_003 + aid) * 2_097_152 + int(counter)) & 0x7FFFFFFFFFFFFFFF)
                u[p] = torch.rand(logits.shape[1:], generator=g, device=self.device)
        u.clamp_(min=1e-20)
        action = torch.argmax(logits - torch.log(-torch.log(u)), dim=-1)
        logp = logp_all.gather(-1, action.unsqueeze(-1)).squeeze(-1)
        return action, logp, ent, value

    def fused_descriptor(self):
        """agx_ppo_net for this architecture, or None when the fused kernels do
        not cover it (then the plain-PyTorch forward / learner run)."""
        if not self.fused or not isinstance(self.spec, ActorCriticSpec) or self.gaussian or self.vector_int:
            return None  # the fused kernels take the categorical MLP actor-critic shapes only
        if self._desc is None:
            from .learner import net_descriptor

            self._desc = net_descriptor(self.spec) or False
        return self._desc or None

    def learn_descriptor(self):
        """The network the fused learn() runs: agx_ppo_net for the compiled
        shapes, else agx_ppo_graph (agx_ppo_learn_graph: any MLP actor-critic
        an architecture mutation produces); None: the plain-PyTorch learner."""
        desc = self.fused_descriptor()
        if (desc is not None or not self.fused or not isinstance(self.spec, ActorCriticSpec) or self.gaussian
                or self.vector_int):
            return desc
        if self._gdesc is None:
            from .learner import graph_descriptor

            self._gdesc = graph_descriptor(self.spec) or False
        return self._gdesc or None

    def eval_descriptor(self):
        """agx_ppo_graph of this network for the evaluation passes: every MLP
        actor-critic, the compiled shapes included, so that a population's
        agents are evaluated together in one launch whatever kernels they train
        on (agx_ppo_eval_multi_persistent).  None: the PyTorch policy step."""
        if not self.fused or not isinstance(self.spec, ActorCriticSpec) or self.gaussian or self.vector_int:
            return None
        if self.fused_descriptor() is None:
            return self.learn_descriptor()  # already the runtime layer list
        if self._edesc is None:
            from .learner import graph_descriptor

            self._edesc = graph_descriptor(self.spec) or False
        return self._edesc or None

    def head_descriptor(self):
        """agx_ppo_graph of a Gaussian / MultiDiscrete / MultiBinary population's
        networks for agx_ppo_act_<stem>_graph.  There is no other policy step
        for such a population: a layer list the kernel does not take is an
        error."""
        if self.head is None:
            return None
        if self._hdesc is None:
            self._hdesc = self.spec.act_descriptor()
            if self._hdesc is None:
                raise _lib.AgxError(f"agx_ppo_act_{self.head.stem}_graph does not take this network: " +
                                    _lib.load(require_gpu=False).agx_last_error().decode(errors="replace"))
        return self._hdesc

    def head_args(self) -> tuple:
        """What the head's entry points take after the descriptor:
        ``spec.log_std``, ``multi_head()``, or nothing."""
        return (self.multi_head(),) if self.multidiscrete else self.head.lead(self.spec)

    def multi_head(self):
        """agx_multi_head of a MultiDiscrete spec's nvec (made once)."""
        if self._mhead is None:
            self._mhead = self.spec.multi_head()
        return self._mhead

    # head_descriptor() / head_learn_descriptor() under the names each head came with: None for any other head
    def gauss_descriptor(self):
        return self.head_descriptor() if self.gaussian else None

    def multi_descriptor(self):
        return self.head_descriptor() if self.multidiscrete else None

    def bern_descriptor(self):
        return self.head_descriptor() if self.multibinary else None

    def gauss_learn_descriptor(self):
        return self.head_learn_descriptor() if self.gaussian else None

    def multi_learn_descriptor(self):
        return self.head_learn_descriptor() if self.multidiscrete else None

    def bern_learn_descriptor(self):
        return self.head_learn_descriptor() if self.multibinary else None

    @torch.no_grad()
    def _head_step(self, obs: torch.Tensor, *, sample: bool, counter: int, action_mask=None):
        """obs [P, N, D] -> (actions [P, N, act_width], log_prob, entropy, value
        [P, N]) of a non-categorical population: float actions [P, N, A]
        (Gaussian), int64 choices [P, N, K] (MultiDiscrete) or 0 / 1 bits
        [P, N, n] (MultiBinary); action_mask uint8 [P, N, L] for the int heads."""
        from .learner import policy_step_head

        P, N, L = self.P, self.N, self.spec.n_actions
        action = torch.empty(P, N, self.act_width, dtype=self.head.dtype, device=self.device)
        logp, ent, value = (torch.empty(P, N, dtype=torch.float32, device=self.device) for _ in range(3))
        policy_step_head(self, obs.contiguous(), N * self.spec.obs_dim, sample=sample, counter=counter,
                         actions=action, log_probs=logp, values=value, entropy=ent, out_agent_stride=N,
                         action_mask=action_mask, mask_agent_stride=N * L)
        return action, logp, ent, value

    def head_learn_descriptor(self):
        """agx_ppo_graph of such a population's networks for its fused learner
        (agx_ppo_learn_<stem>_graph, ``head_args()`` after the descriptor);
        None: a categorical population, ``fused`` off, the head's switch off
        (AGX_GAUSS_FUSED=0, AGX_BERN_FUSED=0; neither ``multi_fused=True`` nor
        AGX_MULTI_FUSED=1), or a layer list agx_ppo_<stem>_graph_check rejects
        — then the autograd learner runs."""
        if self.head is None or not self.fused or not self.head.fused_on(self):
            return None
        if self._hlearn is None:
            self._hlearn = self.spec.learn_descriptor_head() or False
        return self._hlearn or None

    def _fused_learner(self) -> bool:
        """True when learn() runs a fused HIP learner (any head)."""
        return self.learn_descriptor() is not None or self.head_learn_descriptor() is not None

    @torch.no_grad()
    def act_into(self, t: int, actions_flat: torch.Tensor | None = None) -> None:
        """Rollout policy step for slot t: reads obs[:, t], writes actions /
        log_probs / values[:, t] in place (and a contiguous [P*N] copy of the
        actions for the host env step; [P*N*A] floats for a Gaussian population)."""
        if self.head is not None:  # the staging in the head's dtype; slot t's stored masks, when kept
            from .learner import policy_step_head

            self.act_counter += 1
            TN = self.T * self.N
            masks = self.action_masks
            policy_step_head(self, self.obs[:, t], TN * self.spec.obs_dim, sample=True,
                             counter=self.act_counter, actions=self.actions[:, t], log_probs=self.log_probs[:, t],
                             values=self.values[:, t], out_agent_stride=TN, actions_flat=actions_flat,
                             action_mask=None if masks is None else masks[:, t],
                             mask_agent_stride=TN * self.spec.n_actions)
            return
        desc = self.fused_descriptor()
        if desc is None and self.learn_descriptor() is not None:  # a mutated shape: the runtime-shape kernel
            from .learner import policy_step_graph

            self.act_counter += 1
            TN = self.T * self.N
            policy_step_graph(self, self.learn_descriptor(), self.obs[:, t], TN * self.spec.obs_dim, sample=True,
                              counter=self.act_counter, actions=self.actions[:, t], log_probs=self.log_probs[:, t],
                              values=self.values[:, t], out_agent_stride=TN, actions_flat=actions_flat)
            return
        if desc is None:
            self.act_counter += 1
            action, logp, _ent, value = self.act(self.obs[:, t], counter=self.act_counter)
            self.actions[:, t].copy_(action)
            self.values[:, t].copy_(value)
            self.log_probs[:, t].copy_(logp)
            if actions_flat is not None:
                actions_flat.copy_(action.view(-1))
            return
        from .learner import policy_step

        self.act_counter += 1
        TN = self.T * self.N
        policy_step(self, desc, self.obs[:, t], TN * self.spec.obs_dim, sample=True, counter=self.act_counter,
                    actions=self.actions[:, t], log_probs=self.log_probs[:, t], values=self.values[:, t],
                    out_agent_stride=TN, actions_flat=actions_flat)

    @torch.no_grad()
    def store(self, t: int, obs, action, reward, done, value, logp):
        self.obs[:, t].copy_(obs, non_blocking=True)
        self.actions[:, t].copy_(action, non_blocking=True)
        self.rewards[:, t].copy_(reward, non_blocking=True)
        self.dones[:, t].copy_(done, non_blocking=True)
        self.values[:, t].copy_(value, non_blocking=True)
        self.log_probs[:, t].copy_(logp, non_blocking=True)

    def finish_rollout(self, last_obs: torch.Tensor, last_done: torch.Tensor,
                       last_value: torch.Tensor | None = None):
        """Bootstrap value + GAE (+ per-agent advantage statistics).  The fused
        runner computes last_value in its final rollout-step launch."""
        self.rollout_id += 1
        if last_value is None and (self.gaussian or self.vector_int):
            last_value = self.values_of(last_obs)
        elif last_value is None:
            with torch.no_grad():
                _, last_value = self.spec.forward(self.params.data, last_obs)
        if not last_value.is_contiguous():
            last_value = last_value.contiguous()
        if not last_done.is_contiguous():
            last_done = last_done.contiguous()
        key = (last_value.data_ptr(), last_done.data_ptr(), last_value.shape, last_done.dtype,
               *(t.data_ptr() for t in (self.rewards, self.dones, self.values, self.advantages, self.returns,
                                        self.adv_stats, self.gae_ws)))
        if self._gae_launch is not None and self._gae_launch[0] == key:
            self._gae_launch[1](_lib.stream())  # the runner's steady state: one cached launch
            return
        launch = K.gae_launcher(self.rewards, self.dones, self.values, last_value, last_done, self.gamma,
                                self.gae_lambda, True, self.advantages, self.returns, self.adv_stats, self.gae_ws)
        # keep a launcher only for the runner's persistent last_value / last_done
        self._gae_launch = (key, launch, last_value, last_done)

    def action_clip(self):
        """(low, high) device tensors [A] of a Gaussian population's Box
        bounds for the env's copy of the actions at inference, or None."""
        if not self.gaussian or not self.spec.action_low:
            return None
        if getattr(self, "_clip", None) is None:
            self._clip = tuple(torch.tensor(b, dtype=torch.float32, device=self.device)
                               for b in (self.spec.action_low, self.spec.action_high))
        return self._clip

    @torch.no_grad()
    def values_of(self, obs: torch.Tensor) -> torch.Tensor:
        """The critic's values [P, N] of obs [P, N, D] from a Gaussian
        (or MultiDiscrete / MultiBinary) population's policy-step kernel (sample = 0, values only)."""
        from .learner import policy_step_head

        value = torch.empty(self.P, self.N, dtype=torch.float32, device=self.device)
        policy_step_head(self, obs.contiguous(), self.N * self.spec.obs_dim, sample=False, counter=0, values=value,
                         out_agent_stride=self.N)
        return value

    # ------------------------------------------------------------------ #
    def learn(self, prefetch: bool = True, skip_if_set: int | None = None) -> torch.Tensor:
        """One PPO update of every agent; returns the reference's mean_loss per
        agent (device tensor [P], no host sync).  ``prefetch``: draw the next
        learn's permutations right away (the pipelined runner passes False and
        prefetches after pacing the rollout instead)."""
        self.learn_steps += 1
        # the categorical kernels, else the Gaussian graph learner, else (when switched on)
        # the multi-categorical graph learner, else the Bernoulli graph learner
        if self._fused_learner():
            from .learner import fused_learn

            loss = fused_learn(self, skip_if_set=skip_if_set)
            self.last_kl = self._fused.kl
            self.orders.report(self._fused.epochs_run)
            # with target_kl the next learn's shuffles depend on this one's stops
            if prefetch and self.prefetch_perms and self.target_kl is None:
                self.prefetch_permutations()
            return loss
        loss = self._learn_torch()
        self.orders.report(self.last_epochs_run)
        return loss

    def sync_numpy_stream(self) -> None:
        """Apply the correction a target-KL learn owes the global numpy stream."""
        self.orders.settle()

    def check_errors(self) -> None:
        """Raise AgxError if a fused learn() since the last check left an agent's
        update incomplete (a partner workgroup timed out); resets the word.
        Synchronises with the device."""
        w = int(self.err_word.item())
        if w != 0:
            self.err_word.zero_()
            why = []
            if w & 1:  # AGX_LEARN_ERR_TIMEOUT
                why.append("a partner workgroup timed out; the population's parameters are incomplete for this "
                           "learn()")
            if w & 2:  # AGX_LEARN_ERR_PERM
                why.append("a minibatch permutation index was outside [0, S) (the gather prologue substituted "
                           "row 0; this learn() is invalid)")
            raise _lib.AgxError("agx_ppo_learn: " + "; ".join(why or [f"error word {w:#x}"]))

    # ------------------------------------------------------------------ #
    @property
    def heterogeneous(self) -> bool:
        return self._hetero

    @property
    def _hp_dev(self):
        """(batch i32 [P], epochs i32 [P], ent f32 [P]) for the learner, or None
        while every agent shares the population's values (and the partner
        split is sized by that batch: a group split like a larger global
        batch passes its agents' own sizes)."""
        if self._hetero or self.split_batch != self.batch_size:
            return (self.hp_batch_d, self.hp_epochs_d, self.hp_ent_d)
        return None

    def set_agent_hparam(self, p: int, name: str, value) -> None:
        """Set one agent's RL hyperparameter (the HPO mutation of
        mutation.py:413-453 on agent p).  ``learn_step`` would change the
        agent's rollout length, which the lock-step population engine shares
        across agents: it raises NotImplementedError."""
        p = int(p)
        if name == "lr":
            self.opt.lr[p] = float(value)
            self.agent_lr[p] = float(value)
            return
        if name == "batch_size":
            if int(value) < 1:
                raise ValueError("batch_size must be >= 1")
            # a minibatch larger than the rollout is the whole rollout (the
            # reference's indices[start:start + batch_size] slice, ppo.py:843-845):
            # the learner tables hold min(batch, S), the agent keeps its value
            self.agent_batch[p] = int(value)
            self.hp_batch_d[p] = min(int(value), self.S)
        elif name == "update_epochs":
            if int(value) < 1:
                raise ValueError("update_epochs must be >= 1")
            self.agent_epochs[p] = int(value)
            self.hp_epochs_d[p] = int(value)
        elif name == "ent_coef":
            self.agent_ent[p] = float(value)
            self.hp_ent_d[p] = float(value)
        elif name == "learn_step":
            raise NotImplementedError("learn_step is the rollout length every agent of the population engine shares")
        else:
            raise KeyError(f"no per-agent hyperparameter {name!r}")
        self._rederive()

    @property
    def split_batch(self) -> int:
        """The minibatch size that sizes the fused learner's partner split:
        the largest of the GLOBAL population (``global_batch_max``, set by the
        population engine; a shard or a group splits like the whole
        population, so its agents' sums run in the same order)."""
        return min(max(max(self.agent_batch), self.global_batch_max or 0), self.S)

    def set_host_hparams(self, p: int, lr=None, batch_size=None, update_epochs=None, ent_coef=None) -> None:
        """Exact host values of agent p's hyperparameters after a clone whose
        device rows already hold them (a parent from another rank: the
        device tables are f32 / int32, the host lists keep Python floats)."""
        if lr is not None:
            self.agent_lr[p] = float(lr)
        if batch_size is not None:
            self.agent_batch[p] = int(batch_size)
        if update_epochs is not None:
            self.agent_epochs[p] = int(update_epochs)
        if ent_coef is not None:
            self.agent_ent[p] = float(ent_coef)
        self._rederive()

    def reinit_agent_optimizer(self, p: int) -> None:
        """reinit_optimizers for agent p (core/base.py:654-710): a fresh Adam,
        zero moments and step count, the agent's current learning rate."""
        self.opt.exp_avg[p].zero_()
        self.opt.exp_avg_sq[p].zero_()
        self.opt.steps[p] = 0

    def _rederive(self) -> None:
        """Population maxima (they size the learner's workspace and partner
        split) and the heterogeneity flag, from the per-agent lists."""
        self.batch_size = min(max(self.agent_batch), self.S)
        if max(self.agent_epochs) != self.update_epochs:
            self.update_epochs = max(self.agent_epochs)
            self._fused = None      # workspace is sized by the epochs
            self.orders.epochs_changed()
        self._hetero = not (len(set(self.agent_batch)) == 1 and len(set(self.agent_epochs)) == 1
                            and len(set(self.agent_ent)) == 1)

    def after_clone(self, local_parents: list[int] | None) -> None:
        """PopulationSync has copied every cloned row (params, Adam state, lr,
        step, and the per-agent hyperparameter rows).  Single rank: the new
        agent j took local row local_parents[j], mirrored on the host lists;
        several ranks (parents may be remote): re-read the device rows."""
        if local_parents is not None:
            b, e, h, r = list(self.agent_batch), list(self.agent_epochs), list(self.agent_ent), list(self.agent_lr)
            self.agent_batch = [b[q] for q in local_parents]
            self.agent_epochs = [e[q] for q in local_parents]
            self.agent_ent = [h[q] for q in local_parents]
            self.agent_lr = [r[q] for q in local_parents]
        else:
            self.agent_batch = [int(x) for x in self.hp_batch_d.cpu()]
            self.agent_epochs = [int(x) for x in self.hp_epochs_d.cpu()]
            self.agent_ent = [float(x) for x in self.hp_ent_d.cpu()]
            self.agent_lr = [float(x) for x in self.opt.lr.cpu()]
        self._rederive()

    def minibatch_plan(self):
        b = self.batch_size
        return [(s, min(s + b, self.S)) for s in range(0, self.S, b)]

    # minibatch orders: MinibatchOrders (perms.py) owns the draws and the numpy stream
    def permutations(self) -> torch.Tensor:
        """[E, P, S] int64 per-agent minibatch orders for the next learn()."""
        return self.orders.permutations()

    def set_generation_perms(self, block: np.ndarray | None) -> None:
        """A generation's shuffles drawn ahead ([K, E, P, S]); None: draw per learn."""
        self.orders.set_generation_perms(block)

    def prepare_learn(self) -> None:
        """Do now what the next learn() would otherwise do on first use: build
        the fused learner (device workspace) and the pinned permutation
        staging, and draw the permutations.  The pipelined runner calls this
        before launching a persistent rollout: between that launch and the
        host pacing it, the device is waiting for this thread, so nothing
        there may wait for the device — and a hipMalloc / hipHostMalloc, or an
        event sync, can.  Any fused learner: the categorical kernels, the
        Gaussian, the multi-categorical and the Bernoulli graph learner."""
        if self._fused_learner():
            from .learner import learner_stale, make_learner

            if learner_stale(self):
                self._fused = make_learner(self)
        self.orders.alloc_staging()
        if self.prefetch_perms:
            self.prefetch_permutations()

    def prefetch_permutations(self) -> None:
        """Draw the next learn's permutations now, off the critical path."""
        self.orders.prefetch()

    def discard_prefetch(self) -> None:
        """Undo a prefetched numpy draw (and settle the global numpy stream)."""
        self.orders.discard()

    def _learn_torch(self, perms: torch.Tensor | None = None) -> torch.Tensor:
        """Plain-PyTorch fp32 autograd learner over the stacked networks (HIP
        loss and clip + Adam kernels): the numerics cross-check of the fused
        kernel and the path for architectures it does not cover.  Same
        semantics, including target-KL early stop per agent (stopped agents'
        rows are left untouched) and action masks."""
        if perms is None:
            perms = self.permutations()
        K.adv_normalize_(self.advantages, self.adv_stats)
        if not self.heterogeneous:
            return self._learn_torch_group(perms, None, self.batch_size, self.update_epochs, self.ent_coef)
        # per-agent batch / epochs / entropy (HPO mutations): agents sharing all
        # three learn together; the others' rows are left untouched (active mask)
        groups: dict[tuple, list[int]] = {}
        for p in range(self.P):
            groups.setdefault((self.agent_batch[p], self.agent_epochs[p], self.agent_ent[p]), []).append(p)
        out = torch.zeros(self.P, dtype=torch.float32, device=self.device)
        kl = torch.zeros(self.P, dtype=torch.float32, device=self.device)
        ran = torch.zeros(self.P, dtype=torch.int32, device=self.device)
        for (b, e, ent), rows in groups.items():
            loss = self._learn_torch_group(perms, rows, b, e, ent)
            idx = torch.tensor(rows, device=self.device)
            out[idx] = loss[idx]
            kl[idx] = self.last_kl[idx]
            ran[idx] = self.last_epochs_run[idx]
        self.last_kl = kl
        self.last_epochs_run = ran
        return out

    def _categorical_loss(self, ob, ac, masks, idx, rows, image, rollout, gidx, b, ent_coef):
        """Forward of one minibatch per agent and the categorical head's loss
        (log-softmax and entropy in torch, agx_ppo_loss_fwd_bwd)."""
        logits, value = (self.spec.forward(self.params, ob, rows=rows) if image
                         else self.spec.forward(self.params, ob))
        if masks is not None:
            mk = torch.gather(masks, 1, idx.unsqueeze(-1).expand(-1, -1, masks.shape[-1]))
            logits = torch.where(mk.bool(), logits, torch.full_like(logits, -1e8))
        logp_all, ent = categorical(logits)
        logp = logp_all.gather(-1, ac.unsqueeze(-1)).squeeze(-1)
        return _PPOLossFn.apply(logp, value, ent, *rollout, gidx, b, self.clip_coef, self.vf_coef, ent_coef)

    def _learn_torch_group(self, perms, rows, batch_size, epochs, ent_coef) -> torch.Tensor:
        """E epochs x minibatches of ``batch_size`` for the agents in ``rows``
        (None: all agents); -> the reference's mean loss per agent [P]."""
        P, S, D = self.P, self.S, self.spec.obs_dim
        image = not isinstance(self.spec, ActorCriticSpec)
        obs = self.obs.view(P, S, D)
        act = (self.actions.view(P * S, -1) if self.gaussian or self.vector_int else self.actions.view(P, S))
        masks = None if self.action_masks is None else self.action_masks.view(P, S, -1)
        flat_masks = None if masks is None else masks.view(P * S, -1)  # the multi-categorical loss gathers them
        old_logp = self.log_probs.view(-1)
        adv = self.advantages.view(-1)
        ret = self.returns.view(-1)
        old_v = self.values.view(-1)
        base = (torch.arange(P, device=self.device) * S).unsqueeze(1)
        total = torch.zeros(P, dtype=torch.float32, device=self.device)
        kl_sum = torch.zeros(P, dtype=torch.float64, device=self.device)
        n_mb = 0
        member = None
        if rows is not None:
            member = torch.zeros(P, dtype=torch.uint8, device=self.device)
            member[torch.tensor(rows, device=self.device)] = 1
        active = member  # all (member) agents until one stops (u8 [P])
        plan = [(s, min(s + batch_size, S)) for s in range(0, S, batch_size)]
        ran = torch.zeros(P, dtype=torch.int32, device=self.device)  # epochs each agent runs
        for e in range(epochs):
            ran += 1 if active is None else active.int()
            for s0, s1 in plan:
                idx = perms[e][:, s0:s1]  # [P, b]
                ob = torch.gather(obs, 1, idx.unsqueeze(-1).expand(-1, -1, D))
                gidx = (idx + base).reshape(-1).contiguous()
                if self.gaussian:  # the loss kernel gathers the float actions and computes their log-prob
                    mean, value = self.spec.forward(self.params, ob)
                    loss, stats = _PPOGaussLossFn.apply(mean, value, self.spec.log_std_view(self.params), act,
                                                        old_logp, adv, ret, old_v, gidx, s1 - s0, self.clip_coef,
                                                        self.vf_coef, ent_coef)
                elif self.multidiscrete:  # the loss kernel gathers the int64 actions [.., K] and the masks
                    logits, value = self.spec.forward(self.params, ob)
                    loss, stats = _PPOMultiLossFn.apply(logits, value, self.multi_head(), act, flat_masks, old_logp,
                                                        adv, ret, old_v, gidx, s1 - s0, self.clip_coef,
                                                        self.vf_coef, ent_coef)
                elif self.multibinary:  # the loss kernel gathers the int64 bits [.., n] and the masks
                    logits, value = self.spec.forward(self.params, ob)
                    loss, stats = _PPOBernLossFn.apply(logits, value, act, flat_masks, old_logp, adv, ret, old_v,
                                                       gidx, s1 - s0, self.clip_coef, self.vf_coef, ent_coef)
                else:
                    loss, stats = self._categorical_loss(ob, torch.gather(act, 1, idx), masks, idx, rows, image,
                                                         (old_logp, adv, ret, old_v), gidx, s1 - s0, ent_coef)
                self.params.grad.zero_()
                loss.backward()
                self.opt.step(active)
                on = 1.0 if active is None else active.float()
                total += stats[:, 0] * on
                kl_sum += stats[:, 4].double() * (1.0 if active is None else active.double())
                n_mb += 1
            if self.target_kl is not None:
                # np.mean(approx_kl_divs) over every minibatch so far (ppo.py:917-918)
                stop = (kl_sum / n_mb > float(self.target_kl)).to(torch.uint8)
                now = (1 - stop) if active is None else active * (1 - stop)
                if int(now.sum()) == P and active is None:
                    continue
                active = now.contiguous()
                if int(active.sum()) == 0:
                    break
        self.last_kl = (kl_sum / max(n_mb, 1)).float()
        self.last_epochs_run = ran
        return total / (S * epochs)

    # ------------------------------------------------------------------ #
    @torch.no_grad()
    def evaluate(self, obs: torch.Tensor) -> torch.Tensor:
        """Greedy actions (mode of the categorical; the mean of a Gaussian
        policy, [P, N, A]) for fitness evaluation."""
        if self.head is not None:  # the mean; the first arg-max of every component; the mode of every bit
            return self._head_step(obs, sample=False, counter=0)[0]
        logits, _ = self.spec.forward(self.params.data, obs)
        return torch.argmax(logits, dim=-1)

    def n_minibatches(self) -> int:
        return math.ceil(self.S / self.batch_size)

    def n_updates(self) -> int:
        """Minibatch updates of one learn() over the whole population (no early stop)."""
        return sum(e * math.ceil(self.S / b) for b, e in zip(self.agent_batch, self.agent_epochs))

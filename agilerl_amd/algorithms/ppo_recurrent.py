"""``PPO(recurrent=True)`` (agilerl/algorithms/ppo.py with ``recurrent``): a
per-agent path beside the HBM population engine.

The actor (``StochasticActor``) and critic (``ValueNetwork``) are torch modules
on EvolvableLSTM encoders with the reference's module and state-dict names;
the LSTM runs on the fused sequence kernels wherever ``EvolvableLSTM.forward``
takes them (AGX_LSTM, modules/lstm.py).  The rollout lives in a
``RolloutBuffer(recurrent=True)`` in HBM.  ``learn()`` is the truncated-BPTT
loop of ppo.py:923-1111: the advantages normalised over the whole rollout
(agx_gae's statistics + agx_adv_normalize), one agx_bptt_plan, and per
minibatch one agx_bptt_gather, the networks over the padded rows, and
agx_ppo_seq_loss_fwd_bwd (the masked loss with its three gradients, one
``autograd.Function``), then the two gradient clips and Adam.

``get_action`` samples with torch ops on the logits unless the fused step is
switched on (``fused_step=True`` or AGX_RECURRENT_STEP=1; AGX_RECURRENT_STEP=0
always wins): then a policy step, both LSTM encoders, both heads and the draw
from the Philox streams, is one agx_ppo_act_recurrent launch
(include/agx_recurrent.h) wherever its limits hold, and the torch modules run
elsewhere.  The switch is off by default.

``learn()`` runs everything after the LSTMs as torch modules unless the fused
heads are switched on (``fused_learn=True`` or AGX_RECURRENT_LEARN=1;
AGX_RECURRENT_LEARN=0 always wins): then, per minibatch, each encoder's
``nn.LSTM`` runs as ``EvolvableLSTM.forward`` runs it, and the output Linears,
the heads, the log-prob and the entropy of both networks are one
agx_recurrent_heads_forward launch with a two-launch backward
(include/agx_recurrent_heads.h) wherever the limits hold.  Off by default.

Action spaces: Discrete, 1-D Box, 1-D MultiDiscrete and 1-D MultiBinary, each
on both paths; the last two on a CUDA device only (on the CPU the agent keeps
refusing them, as it did before they existed).  Image / Dict observations and
``squash_output`` raise.

``share_encoders=True`` (the reference's default, CUDA only; the CPU keeps
refusing it): both networks are built on ``shared_encoder``, the actor's encoder
is the live one and the critic's head reads the actor's latent
(ppo.py:430-442), so a step and a minibatch run one LSTM, the hidden state is
the ``shared_encoder_h`` / ``_c`` pair, and the encoder's gradient carries the
value loss's share.  The critic's own encoder is a non-trainable copy that is
never run: synced from the actor's at construction, after ``learn()`` and after
``load_state_dict``, so ``state_dict()`` has the reference's keys.  With the
switches on, the step is agx_ppo_act_recurrent_shared and the heads are
agx_recurrent_heads_forward_shared / _backward_shared: one workgroup per row
tile runs both heads off the one latent.
"""

from __future__ import annotations

import copy
import os
import warnings

import numpy as np
import torch
from torch.autograd.function import once_differentiable
from torch.nn.utils import clip_grad_norm_

from .. import kernels as K
from ..components.rollout_buffer import RolloutBuffer
from ..networks.actors import StochasticActor
from ..networks.base import as_config, mlp_net_config
from ..networks.value_networks import ValueNetwork
from .ppo import PPO


class SeqLossFn(torch.autograd.Function):
    """(logp, value, entropy [rows]; the minibatch's valid rows and rollout values) -> (loss, stats [8])."""

    @staticmethod
    def forward(ctx, logp, value, entropy, valid_row, old_logp, adv, ret, old_value, clip_coef, vf_coef, ent_coef):
        g_logp, g_value, g_entropy, stats = K.ppo_seq_loss_fwd_bwd(
            logp.detach().contiguous(), value.detach().contiguous(), entropy.detach().contiguous(), valid_row,
            old_logp, adv, ret, old_value, clip_coef, vf_coef, ent_coef)
        ctx.save_for_backward(g_logp, g_value, g_entropy)
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        g_logp, g_value, g_entropy = ctx.saved_tensors
        return (g_loss * g_logp, g_loss * g_value, g_loss * g_entropy) + (None,) * 8


class HeadsFn(torch.autograd.Function):
    """(actor, critic, actions, mask; both networks' top-layer LSTM outputs [rows, H]; the parameters of
    kernels.recurrent_heads_params) -> (log_prob, entropy, value [rows])."""

    @staticmethod
    def forward(ctx, actor, critic, actions, mask, h_actor, h_critic, *params):
        # h_critic is None for a pair that shares one encoder: one h_top, and one dh_top on the way back
        h_top = tuple(h.detach().contiguous() for h in (h_actor, h_critic) if h is not None)
        logp, entropy, value, saved = K.recurrent_heads_forward(actor, critic, h_top, actions, mask)
        ctx.nets, ctx.mask = (actor, critic), mask
        ctx.save_for_backward(*h_top, actions, saved)
        return logp, entropy, value

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logp, g_entropy, g_value):
        *h_top, actions, saved = ctx.saved_tensors
        ups = [torch.zeros(h_top[0].shape[0], device=h_top[0].device) if g is None else g.float().contiguous()
               for g in (g_logp, g_entropy, g_value)]
        dh_actor, dh_critic, grads = K.recurrent_heads_backward(*ctx.nets, tuple(h_top), actions, ctx.mask, saved,
                                                                *ups)
        return (None, None, None, None, dh_actor, dh_critic, *grads)


class RecurrentPPO(PPO):
    # the population view's descriptors give way to plain attributes
    lr = batch_size = update_epochs = ent_coef = learn_step = rollout_buffer = None
    can_mutate_architecture = False

    def __init__(self, observation_space, action_space, index: int = 0, hp_config=None, net_config=None,
                 batch_size: int = 64, lr: float = 1e-4, learn_step: int = 2048, gamma: float = 0.99,
                 gae_lambda: float = 0.95, mut=None, action_std_init: float = 0.0, clip_coef: float = 0.2,
                 ent_coef: float = 0.01, vf_coef: float = 0.5, max_grad_norm: float = 0.5,
                 target_kl: float | None = None, normalize_images: bool = True, update_epochs: int = 4,
                 actor_network=None, critic_network=None, share_encoders: bool = True, num_envs: int = 1,
                 use_rollout_buffer: bool = True, rollout_buffer_config=None, recurrent: bool = True, device="cuda",
                 accelerator=None, wrap: bool = True, bptt_sequence_type=None, max_seq_len=None,
                 fused_step: bool = False, fused_learn: bool = False) -> None:
        from ..hpo.registry import MutationRegistry

        if not use_rollout_buffer:
            raise ValueError("use_rollout_buffer must be True if recurrent=True.")
        if actor_network is not None or critic_network is not None:
            raise NotImplementedError("custom actor/critic modules: use net_config networks")
        if share_encoders and torch.device(device).type != "cuda":
            # as before the shared form existed: off the GPU the agent is built with separate encoders only
            raise NotImplementedError("agx recurrent PPO: share_encoders=True needs a CUDA device; on the CPU pass "
                                      "share_encoders=False")
        assert isinstance(batch_size, int) and batch_size >= 1, "Batch size must be an integer greater than or equal to one."
        assert lr > 0, "Learning rate must be greater than zero."
        assert action_std_init >= 0, "Action standard deviation must be greater than or equal to zero."
        assert isinstance(learn_step, int) and learn_step >= 1, "Learn step rate must be an integer greater than or equal to one."
        K.bptt_sequence_type(bptt_sequence_type)  # "bptt_sequence_type must be a BPTTSequenceType enum value."
        self.observation_space, self.action_space = observation_space, action_space
        self.index, self.net_config, self.mut = index, net_config, mut
        self.batch_size, self.lr, self.learn_step = batch_size, lr, learn_step
        self.gamma, self.gae_lambda = gamma, gae_lambda
        self.action_std_init, self.clip_coef, self.ent_coef, self.vf_coef = action_std_init, clip_coef, ent_coef, vf_coef
        self.max_grad_norm, self.target_kl, self.update_epochs = max_grad_norm, target_kl, update_epochs
        self.num_envs, self.share_encoders, self.recurrent = num_envs, bool(share_encoders), True
        self.use_rollout_buffer = True
        self.rollout_buffer_config = dict(rollout_buffer_config or {})
        self.max_seq_len, self.bptt_sequence_type = max_seq_len, bptt_sequence_type
        self.device = torch.device(device)
        if (K.recurrent_head(action_space) or (0,))[0] >= K.HEAD_MULTI and self.device.type != "cuda":
            # as before this change: off the GPU the agent is built for Discrete and Box only
            raise NotImplementedError("agx recurrent PPO: MultiDiscrete / MultiBinary actions need a CUDA device")
        self.training = True
        self.registry = MutationRegistry(hp_config)
        self.scores, self.fitness, self.steps = [], [], [0]
        self.hidden_state = None
        self.fused_step, self.fused_learn = bool(fused_step), bool(fused_learn)
        self._act_seed, self._act_counter = None, 0  # the Philox key of the fused step: drawn on its first call

        cfg = dict(as_config(net_config) or {})
        critic_cfg = copy.deepcopy(cfg)
        head = as_config(cfg.get("head_config"))
        if head is not None:  # ppo.py:292-300
            critic_head = copy.deepcopy(head)
            critic_head["output_activation"] = None
            critic_cfg.pop("squash_output", None)
        else:
            critic_head = mlp_net_config([16])
        critic_cfg["head_config"] = critic_head
        names = ("shared_encoder",) * 2 if self.share_encoders else ("actor_encoder", "critic_encoder")  # ppo.py:308-316
        self.actor = StochasticActor(observation_space, action_space, action_std_init=action_std_init,
                                     device=self.device, recurrent=True, encoder_name=names[0], **cfg)
        self.critic = ValueNetwork(observation_space, device=self.device, recurrent=True,
                                   encoder_name=names[1], **critic_cfg)
        if self.share_encoders:
            # The actor's encoder is the live one.  The critic's is a copy that is never run: it takes no gradient,
            # is not in the optimiser, and is there so that state_dict() has the reference's keys.
            self.critic.encoder.requires_grad_(False)
            self.sync_shared_encoder()
        # the distribution: kernels.HEAD_*, and how many columns a row of stored actions has
        self.head_kind, _, _, self.action_cols = K.recurrent_head(action_space)
        self.discrete = self.head_kind == K.HEAD_DISCRETE
        self.reinit_optimizers()
        self.create_rollout_buffer()

    # ---- the pieces of the reference's agent ----------------------------------
    def reinit_optimizers(self, optimizer=None) -> None:
        params = list(self.actor.parameters()) + [p for p in self.critic.parameters() if p.requires_grad]
        self.optimizer = torch.optim.Adam(params, lr=self.lr)

    @torch.no_grad()
    def sync_shared_encoder(self) -> None:
        """share_encoders: the critic's encoder entries take the actor's values (after every change of those)."""
        if self.share_encoders:
            for dst, src in zip(self.critic.encoder.state_dict().values(), self.actor.encoder.state_dict().values()):
                dst.copy_(src)

    def create_rollout_buffer(self) -> None:
        """ppo.py:360-378."""
        self.rollout_buffer = RolloutBuffer(capacity=-(self.learn_step // -self.num_envs),
                                            observation_space=self.observation_space,
                                            action_space=self.action_space, device=self.device,
                                            num_envs=self.num_envs, gae_lambda=self.gae_lambda, gamma=self.gamma,
                                            recurrent=True,
                                            hidden_state_architecture=self.get_hidden_state_architecture(),
                                            max_seq_len=self.max_seq_len, bptt_sequence_type=self.bptt_sequence_type,
                                            **self.rollout_buffer_config)

    def get_initial_hidden_state(self, num_envs: int = 1) -> dict[str, torch.Tensor]:
        """ppo.py:519-525: with a shared encoder the actor's state is the only one."""
        if self.share_encoders:
            return self.actor.initialize_hidden_state(batch_size=num_envs)
        return {**self.actor.initialize_hidden_state(batch_size=num_envs),
                **self.critic.initialize_hidden_state(batch_size=num_envs)}

    def get_hidden_state_architecture(self) -> dict[str, tuple[int, ...]]:
        return {k: tuple(v.shape) for k, v in self.get_initial_hidden_state(self.num_envs).items()}

    def architecture_mutation(self, new_layer_prob: float, rng):
        return None

    def mutation_hook(self) -> None:
        self.create_rollout_buffer()

    def state_dict(self) -> dict[str, torch.Tensor]:
        return {f"{net}.{k}": v for net in ("actor", "critic") for k, v in getattr(self, net).state_dict().items()}

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict: bool = True) -> None:
        for net in ("actor", "critic"):
            getattr(self, net).load_state_dict({k[len(net) + 1:]: v for k, v in state_dict.items()
                                                if k.startswith(net + ".")}, strict=strict)
        self.sync_shared_encoder()

    def save_checkpoint(self, path: str) -> None:
        raise NotImplementedError("agx recurrent PPO: checkpoints are not written yet (state_dict / load_state_dict)")

    def load_checkpoint(self, path: str) -> None:
        raise NotImplementedError("agx recurrent PPO: checkpoints are not read yet (state_dict / load_state_dict)")

    # ---- acting -----------------------------------------------------------------
    def preprocess_observation(self, obs) -> torch.Tensor:
        if not isinstance(obs, torch.Tensor):
            obs = torch.as_tensor(np.asarray(obs), dtype=torch.float32)
        return obs.to(self.device, torch.float32).reshape(-1, *self.observation_space.shape)

    def _get_action_and_values(self, obs, action_mask=None, hidden_state=None, *, sample: bool = True):
        """ppo.py:400-492.  Separate encoders: the actor and the critic take the states of their own keys.  A shared
        encoder (ppo.py:430-442): the critic's head reads the actor's latent."""
        if hidden_state is None:
            raise ValueError("recurrent PPO acts on a hidden state (get_initial_hidden_state)")
        if self.share_encoders:
            latent, next_hidden = self.actor.extract_features(obs, hidden_state=hidden_state)
            action, log_prob, entropy = self.actor.forward_head(latent, action_mask=action_mask, sample=sample)
            return action, log_prob, entropy, self.critic.forward_head(latent).squeeze(-1), next_hidden
        actor_h = {k: v for k, v in hidden_state.items() if k.startswith("actor_encoder")}
        critic_h = {k: v for k, v in hidden_state.items() if k.startswith("critic_encoder")}
        latent, next_actor = self.actor.extract_features(obs, hidden_state=actor_h)
        action, log_prob, entropy = self.actor.forward_head(latent, action_mask=action_mask, sample=sample)
        values, next_critic = self.critic(obs, hidden_state=critic_h)
        return action, log_prob, entropy, values.squeeze(-1), {**next_actor, **next_critic}

    def fused_step_on(self) -> bool:
        env = os.environ.get("AGX_RECURRENT_STEP")
        return env != "0" and (self.fused_step or env == "1")

    def fused_policy_step(self, obs, action_mask=None, hidden_state=None, *, sample: bool = True, reset=None,
                          out=None, store_hidden=None, store_obs=None):
        """One agx_ppo_act_recurrent launch over preprocessed ``obs`` (kernels.ppo_act_recurrent's dict), or None
        with the switch off or where the kernel does not apply.  A sampled step advances the agent's counter."""
        if not self.fused_step_on() or hidden_state is None or obs.device.type != "cuda":
            return None
        if self._act_seed is None:
            self._act_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        res = K.ppo_act_recurrent(self.actor, self.critic, obs.reshape(obs.shape[0], -1), hidden_state,
                                  sample=sample, seed=self._act_seed, counter=self._act_counter + 1,
                                  mask=action_mask, reset=reset, out=out, store_hidden=store_hidden,
                                  store_obs=store_obs)
        if res is not None and sample:
            self._act_counter += 1
        return res

    def host_action(self, action: np.ndarray) -> np.ndarray:
        """A step's actions [N, columns] as ``get_action`` returns them: int64 [N] (Discrete) or [N, K]
        (MultiDiscrete), [N, n] of the space's dtype (MultiBinary), float32 [N, A] (Box)."""
        if self.head_kind == K.HEAD_DISCRETE:
            return action.reshape(action.shape[0]).astype(np.int64)
        if self.head_kind == K.HEAD_MULTI:
            return action.astype(np.int64)
        if self.head_kind == K.HEAD_BERNOULLI:
            return action.astype(self.action_space.dtype)
        return action

    def evaluate_actions(self, obs, actions, hidden_state=None, action_mask=None):
        """-> (log_prob, entropy, values) of ``actions`` (ppo.py:529-565); with [layers, B, H] states and
        B * L rows of observations the rows are B sequences of L steps."""
        obs = self.preprocess_observation(obs)
        _, _, entropy, values, _ = self._get_action_and_values(obs, action_mask, hidden_state, sample=False)
        return self.actor.action_log_prob(actions), entropy, values

    def get_action(self, obs, action_mask=None, hidden_state=None, *args, **kwargs):
        """-> (action, log_prob, entropy, value, next hidden state) (ppo.py:567-633)."""
        obs = self.preprocess_observation(obs)
        res = self.fused_policy_step(obs, action_mask, hidden_state)
        if res is not None:  # one launch, then one read of what it returned
            host = torch.cat([res["actions"].reshape(-1), res["log_probs"], res["entropy"], res["values"]]).cpu()
            n = obs.shape[0]
            action = self.host_action(host[:-3 * n].reshape(n, -1).numpy())
            if not self.training and self.head_kind == K.HEAD_BOX:
                action = np.clip(action, self.action_space.low, self.action_space.high)
            log_prob, entropy, values = host[-3 * n:].reshape(3, n).numpy()
            return action, log_prob, entropy, values, res["hidden"]
        with torch.no_grad():
            action, log_prob, entropy, values, next_hidden = self._get_action_and_values(obs, action_mask,
                                                                                         hidden_state, sample=True)
        action = self.host_action(action.cpu().numpy())
        if not self.training and self.head_kind == K.HEAD_BOX:
            action = np.clip(action, self.action_space.low, self.action_space.high)
        return action, log_prob.cpu().numpy(), entropy.cpu().numpy(), values.cpu().numpy(), next_hidden

    def bootstrap_value(self, obs, hidden_state) -> torch.Tensor:
        """The value [N] of ``obs`` under ``hidden_state`` without a draw: the rollout's last value."""
        obs = self.preprocess_observation(obs)
        res = self.fused_policy_step(obs, None, hidden_state, sample=False)
        if res is not None:
            return res["values"]
        with torch.no_grad():
            return self._get_action_and_values(obs, hidden_state=hidden_state, sample=False)[3]

    # ---- learning ---------------------------------------------------------------
    def fused_learn_on(self) -> bool:
        env = os.environ.get("AGX_RECURRENT_LEARN")
        return env != "0" and (self.fused_learn or env == "1")

    def fused_heads(self, obs, actions, hidden_state, action_mask=None):
        """(log_prob, entropy, values) of ``evaluate_actions`` with everything after the LSTMs on the head kernels
        (HeadsFn), or None with the switch off or where they do not apply."""
        if not self.fused_learn_on() or not isinstance(actions, torch.Tensor) or actions.device.type != "cuda":
            return None
        params = K.recurrent_heads_params(self.actor, self.critic)
        if params is None or (action_mask is not None and self.head_kind == K.HEAD_BOX):
            return None
        obs = self.preprocess_observation(obs)
        h_top = [net.encoder.lstm_output(obs, hidden_state)[0]
                 for net in ((self.actor,) if self.share_encoders else (self.actor, self.critic))]
        if any(h.dim() != 2 or h.dtype != torch.float32 for h in h_top):
            return None
        h_top += [None] * (2 - len(h_top))  # a shared encoder: one LSTM run, no h_top of the critic's
        actions = actions.to(torch.float32).contiguous()
        if actions.shape != ((h_top[0].shape[0],) if self.discrete else (h_top[0].shape[0], self.action_cols)):
            return None
        return HeadsFn.apply(self.actor, self.critic, actions, action_mask, *h_top, *params)

    def bptt_loss(self, padded: dict, unpadded: dict):
        """One minibatch of get_minibatch_sequences -> (loss, stats [8]) (ppo.py:964-1050): the networks over
        every padded row, the masked loss in one kernel."""
        actions = padded["actions"].squeeze(-1) if self.discrete else padded["actions"]
        fused = self.fused_heads(padded["observations"], actions, padded["initial_hidden_states"],
                                 padded.get("action_masks"))
        logp, entropy, values = fused if fused is not None else self.evaluate_actions(
            padded["observations"], actions, hidden_state=padded["initial_hidden_states"],
            action_mask=padded.get("action_masks"))
        return SeqLossFn.apply(logp, values, entropy, unpadded["valid_row"], unpadded["log_probs"],
                               unpadded["advantages"], unpadded["returns"], unpadded["values"],
                               float(self.clip_coef), float(self.vf_coef), float(self.ent_coef))

    def learn(self, experiences=None) -> float:
        if experiences is not None:
            raise ValueError("recurrent PPO learns from its rollout buffer (use_rollout_buffer=True)")
        buf = self.rollout_buffer
        buf.normalize_advantages()  # over the whole valid buffer, before planning (ppo.py:935-944)
        buf.prepare_sequence_tensors()
        params_a, params_c = list(self.actor.parameters()), list(self.critic.parameters())
        mean_loss, updates = 0.0, 0
        for epoch in range(int(self.update_epochs)):
            epoch_kl, last_kl = [], None
            for padded, unpadded in buf.get_minibatch_sequences(int(self.batch_size)):
                loss, stats = self.bptt_loss(padded, unpadded)
                self.optimizer.zero_grad()
                loss.backward()
                clip_grad_norm_(params_a, self.max_grad_norm)
                clip_grad_norm_(params_c, self.max_grad_norm)
                self.optimizer.step()
                host = stats.cpu()  # the loss and the KL in one read
                mean_loss += float(host[0])
                updates += 1
                if self.target_kl is not None:
                    last_kl = float(host[4])
                    epoch_kl.append(last_kl)
                    if last_kl > self.target_kl:
                        warnings.warn(f"Epoch {epoch}, Minibatch: KL divergence {last_kl:.4f} exceeded target "
                                      f"{self.target_kl}. Stopping update for this epoch.", stacklevel=2)
                        break
            # ppo.py:1086-1109: the epoch's mean KL, or the minibatch that broke the inner loop, ends the update
            if self.target_kl is not None and epoch_kl and (np.mean(epoch_kl) > self.target_kl
                                                            or last_kl > self.target_kl):
                break
        self.sync_shared_encoder()
        return mean_loss / max(1e-8, updates)

    # ---- evaluation ---------------------------------------------------------------
    def _test_loops(self, env, num_envs: int, max_steps: int | None, loop: int) -> float:
        """ppo.py:1145-1289: the hidden state is carried and reset for the envs that finish."""
        self.actor.eval()
        self.critic.eval()
        try:
            rewards = []
            for _ in range(loop):
                obs, info = env.reset()
                scores, completed = np.zeros(num_envs), np.zeros(num_envs)
                finished = np.zeros(num_envs, dtype=bool)
                hidden = self.get_initial_hidden_state(num_envs)
                step = 0
                while not np.all(finished):
                    mask = info.get("action_mask") if isinstance(info, dict) else None
                    action, _, _, _, hidden = self.get_action(obs, action_mask=mask, hidden_state=hidden)
                    obs, reward, term, trunc, info = env.step(action)
                    step += 1
                    scores += np.asarray(reward).reshape(num_envs)
                    done = np.logical_or(term, trunc).reshape(num_envs)
                    newly = np.logical_or(done, max_steps is not None and step == max_steps) & ~finished
                    if np.any(newly):
                        reset_hidden_state(hidden, self.get_initial_hidden_state(num_envs), newly)
                        completed[newly] = scores[newly]
                        finished[newly] = True
                rewards.append(float(np.mean(completed)))
        finally:
            self.actor.train()
            self.critic.train()
        mean_fit = float(np.mean(rewards))
        self.fitness.append(mean_fit)
        return mean_fit


def reset_hidden_state(hidden: dict, initial: dict, finished) -> None:
    """In place: the states of the envs flagged in ``finished`` go back to the initial state
    (rollouts/on_policy.py:152-169)."""
    sel = torch.as_tensor(np.asarray(finished, dtype=bool))
    for key, h in hidden.items():
        sel_dev = sel.to(h.device)
        h[:, sel_dev, :] = initial[key][:, sel_dev, :]

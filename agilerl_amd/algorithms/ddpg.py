"""Drop-in ``DDPG`` (agilerl/algorithms/ddpg.py:30-514) for Box observations
(vectors) and Box actions, and the machinery it shares with ``TD3``
(algorithms/td3.py): one deterministic actor, one or two Q(s, a) critics,
a target copy of each.

Networks are the reference's: ``DeterministicActor`` (EvolvableMLP encoder +
"actor" head, Tanh output) and ``ContinuousQNetwork`` (encoder without
LayerNorm + "value" head on [latent, a]), each eval network with its own
``torch.optim.Adam``.  Of an update, the two steps between the target
networks' forwards run in libagx (include/agx_td3.h): the target-policy
smoothing max(min(mu'(s') + clamp(noise, -c, c), high), low) is one
``agx_td3_smooth_actions`` launch, and y = r + (1 - d) gamma min(Q1', Q2'),
the MSE loss(es) and their gradients one ``agx_td3_critic_target`` launch.
Every optimizer step and every soft update is one launch per network over
flat parameter buffers (``FlatLearnState``: agx_clip_adam without a clip, as
the reference does not clip, and agx_polyak), the torch optimizers staying
the source of truth for state_dict / checkpoints / clones.

Exploration noise (``action_noise`` / ``reset_action_noise``) is drawn on the
host from the global numpy generator with the reference's formulas, so a
seeded run draws what the reference draws.

Outside this path (NotImplementedError): ``share_encoders=True``, custom
actor / critic modules, observation spaces other than vectors.
"""

from __future__ import annotations

import copy
import warnings
from typing import Any

import numpy as np
import torch

from .. import kernels as K
from ..networks import ContinuousQNetwork, DeterministicActor
from ..networks.base import as_config, mlp_net_config
from . import checkpoint as C
from .evolvable import EvolvableAgentMixin, NetGroup
from .flat_state import flat_state
from .offpolicy import MSECriticLoss, _evaluate, batch


def _arch(net) -> dict:
    """What architecture mutations change of an MLP-encoder network."""
    return {"latent_dim": int(net.latent_dim), "encoder": [int(h) for h in net.encoder.hidden_size],
            "head": [int(h) for h in net.head_net.hidden_size]}


def _set_arch(net, arch: dict) -> None:
    if _arch(net) == arch:
        return
    old = net.latent_dim
    net.latent_dim = int(arch["latent_dim"])
    net.encoder.hidden_size = [int(h) for h in arch["encoder"]]
    net.head_net.hidden_size = [int(h) for h in arch["head"]]
    net.recreate_network(old)


def save_arch(agent, ck: dict) -> None:
    """Into a checkpoint being saved: the architecture of every network of the
    agent's groups (MLP encoders), so a mutated agent loads into a fresh one."""
    ck["network_arch"] = {n: _arch(getattr(agent, n)) for g in agent._groups for n in g[:2] if n}


def restore_arch(agent, ck: dict) -> None:
    """Take it back, before the state dicts are loaded: networks rebuilt where
    they differ, then fresh optimizers over the (possibly rebuilt) parameters."""
    for n, arch in ck.get("network_arch", {}).items():
        _set_arch(getattr(agent, n), arch)
    agent.reinit_optimizers()


_ACTOR = NetGroup("actor", "actor_target", "actor_optimizer", "lr_actor")


class _DeterministicPolicyGradient(EvolvableAgentMixin, C.TorchCheckpointMixin):
    """DDPG / TD3: the actor group, then one group per critic."""

    _ckpt_spaces = False
    #: attributes beyond checkpoint.HP_NAMES that a checkpoint carries
    _CKPT_EXTRA = ("lr_actor", "lr_critic", "policy_freq", "learn_counter", "O_U_noise", "vect_noise_dim", "theta",
                   "dt")
    _CKPT_ARRAYS = ("expl_noise", "mean_noise", "current_noise")
    _bounds = None  # (action_low, action_high) on the device, made at the first update

    def _setup(self, observation_space, action_space, O_U_noise, expl_noise, vect_noise_dim, mean_noise, theta, dt,
               index, hp_config, net_config, batch_size, lr_actor, lr_critic, learn_step, gamma, tau,
               normalize_images, mut, policy_freq, custom_networks, share_encoders, device, wrap) -> None:
        name = self.algo
        assert learn_step >= 1, "Learn step must be greater than or equal to one."
        assert isinstance(learn_step, int), "Learn step rate must be an integer."
        assert hasattr(action_space, "low") and hasattr(action_space, "high") and not hasattr(action_space, "n"), \
            f"{name} only supports continuous action spaces."
        self.action_dim = int(action_space.shape[0])
        assert (isinstance(expl_noise, (float, int))) or (
            isinstance(expl_noise, np.ndarray) and expl_noise.shape == (vect_noise_dim, self.action_dim)), \
            "Exploration action noise rate must be a float, or an array of size action_dim"
        if isinstance(expl_noise, (float, int)):
            assert expl_noise >= 0, "Exploration noise must be greater than or equal to zero."
        assert isinstance(batch_size, int), "Batch size must be an integer."
        assert batch_size >= 1, "Batch size must be greater than or equal to one."
        assert isinstance(lr_actor, float), "Actor learning rate must be a float."
        assert lr_actor > 0, "Actor learning rate must be greater than zero."
        assert isinstance(lr_critic, float), "Critic learning rate must be a float."
        assert lr_critic > 0, "Critic learning rate must be greater than zero."
        assert isinstance(gamma, (float, int, torch.Tensor)), "Gamma must be a float."
        assert isinstance(tau, float), "Tau must be a float."
        assert tau > 0, "Tau must be greater than zero."
        assert isinstance(policy_freq, int), "Policy frequency must be an integer."
        assert policy_freq >= 1, "Policy frequency must be greater than or equal to one."
        assert isinstance(wrap, bool), "Wrap models flag must be boolean value True or False."
        if any(n is not None for n in custom_networks):
            raise NotImplementedError("custom actor/critic modules: use net_config (MLP) networks")
        if share_encoders:
            raise NotImplementedError("share_encoders=True: the actor and the critics keep their own encoders")
        if hasattr(observation_space, "spaces") or len(getattr(observation_space, "shape", ())) != 1:
            raise NotImplementedError(f"agx {name} takes vector (1-D Box) observation spaces")

        self.observation_space, self.action_space = observation_space, action_space
        self.index, self.mut, self.net_config = index, mut, net_config
        self.batch_size, self.lr_actor, self.lr_critic = batch_size, lr_actor, lr_critic
        self.learn_step, self.gamma, self.tau, self.policy_freq = learn_step, gamma, tau, policy_freq
        self.normalize_images, self.wrap, self.share_encoders = normalize_images, wrap, share_encoders
        self.O_U_noise, self.vect_noise_dim, self.theta, self.dt = O_U_noise, vect_noise_dim, theta, dt
        self.device = torch.device(device)
        self.obs_dim = int(observation_space.shape[0])
        self.expl_noise = expl_noise if isinstance(expl_noise, np.ndarray) else \
            expl_noise * np.ones((vect_noise_dim, self.action_dim))
        self.mean_noise = mean_noise if isinstance(mean_noise, np.ndarray) else \
            mean_noise * np.ones((vect_noise_dim, self.action_dim))
        self.current_noise = np.zeros((vect_noise_dim, self.action_dim))
        self.learn_counter = 0
        self.action_low = torch.as_tensor(np.asarray(action_space.low), dtype=torch.float32)
        self.action_high = torch.as_tensor(np.asarray(action_space.high), dtype=torch.float32)
        self.training = True
        self.scores: list[float] = []
        self.fitness: list[float] = []
        self.steps: list[int] = [0]

        # network construction (td3.py:242-303, ddpg.py:228-287)
        net_config = copy.deepcopy(as_config(net_config) or {})
        encoder_config = as_config(net_config.get("encoder_config"))
        if encoder_config is not None:
            if "hidden_size" in encoder_config:
                if encoder_config.get("layer_norm", False):
                    warnings.warn(f"Layer normalization is not supported for the encoder of {name} networks. "
                                  "Disabling it. See GitHub PR for more details: "
                                  "https://github.com/AgileRL/AgileRL/pull/469", stacklevel=3)
                encoder_config["layer_norm"] = False
        else:
            encoder_config = mlp_net_config([64, 64], output_activation="ReLU", output_vanish=False,
                                            layer_norm=False)
        net_config["encoder_config"] = encoder_config
        head_config = as_config(net_config.get("head_config"))
        if head_config is not None:
            critic_head_config = copy.deepcopy(head_config)
            critic_head_config["output_activation"] = None
        else:
            critic_head_config = mlp_net_config([64])
        critic_net_config = copy.deepcopy(net_config)
        critic_net_config["head_config"] = critic_head_config

        def create_actor() -> DeterministicActor:
            return DeterministicActor(observation_space, action_space, device=self.device,
                                      **copy.deepcopy(net_config))

        def create_critic() -> ContinuousQNetwork:
            return ContinuousQNetwork(observation_space, action_space, device=self.device,
                                      **copy.deepcopy(critic_net_config))

        # construction order of the reference: actor, its target, then each critic and its target
        self.actor, self.actor_target = create_actor(), create_actor()
        for g in self._groups[1:]:
            setattr(self, g.net, create_critic())
            setattr(self, g.target, create_critic())
        for net, target, _ in self._triples():
            getattr(self, target).load_state_dict(getattr(self, net).state_dict())
        # the networks' own generators (EvolvableModule.rng, shared with their
        # modules; seeded from the agent's initial index so a run is reproducible)
        self.actor.rng = np.random.default_rng((0x5EED, int(index), 0))
        for i, g in enumerate(self._groups[1:]):
            getattr(self, g.net).rng = np.random.default_rng((0x5EEE, int(index), i))
        self.reinit_optimizers()
        self._init_registry(hp_config)

    # ---- architecture mutation (hpo/mutation.py:829-885) ----------------------
    def architecture_mutation(self, new_layer_prob: float, rng) -> str | None:
        """_architecture_mutate_single: a method sampled from the actor's
        table with ``rng`` (Mutations.rng) and applied to the actor; the
        method it applied, with its mutation dict, to every critic whose
        table has it; every target re-made from its eval network
        (reinit_shared_networks, :104-160).  -> the applied method or None."""
        applied, mut_dict = self.actor.apply_mutation_dict(self.actor.sample_mutation_method(new_layer_prob, rng))
        for g in self._groups[1:]:
            critic = getattr(self, g.net)
            if applied in critic.mutation_methods:
                critic.apply_mutation_dict(applied, mut_dict)
        for net, target, _ in self._triples():
            setattr(self, target, copy.deepcopy(getattr(self, net)))
        return applied

    # ---- acting (td3.py:392-460) ----------------------------------------------
    def set_training_mode(self, training: bool) -> None:
        self.training = training

    def _obs(self, obs) -> torch.Tensor:
        x = obs if isinstance(obs, torch.Tensor) else torch.as_tensor(np.asarray(obs))
        return x.to(self.device).to(torch.float32).reshape(-1, self.obs_dim)

    def get_action(self, obs, training: bool = True, *args: Any, **kwargs: Any) -> np.ndarray:
        """The actor's output plus exploration noise, clipped to [-1, 1]
        (training: the raw action the replay buffer stores), or the output
        rescaled to the action space's bounds."""
        self.actor.eval()
        with torch.no_grad():
            action = self.actor(self._obs(obs))
        self.actor.train()
        if training:
            return (action.cpu().numpy() + self.action_noise()).clip(-1, 1)
        return DeterministicActor.rescale_action(action.cpu(), self.action_low, self.action_high,
                                                 self.actor.output_activation).numpy()

    def action_noise(self) -> np.ndarray:
        """Ornstein-Uhlenbeck or Gaussian exploration noise, f32
        [vect_noise_dim, action_dim], from the global numpy generator."""
        if self.O_U_noise:
            noise = (self.current_noise + self.theta * (self.mean_noise - self.current_noise) * self.dt
                     + self.expl_noise * np.sqrt(self.dt)
                     * np.random.normal(size=(self.vect_noise_dim, self.action_dim)))
            self.current_noise = noise
        else:
            noise = np.random.normal(self.mean_noise, self.expl_noise, size=(self.vect_noise_dim, self.action_dim))
        return noise.astype(np.float32)

    def reset_action_noise(self, indices) -> None:
        self.current_noise[indices] = self.mean_noise[indices]

    # ---- learning (td3.py:462-551, ddpg.py:422-498) ---------------------------
    def learn(self, experiences, noise_clip: float = 0.5, policy_noise: float = 0.2) -> tuple[float | None, float]:
        """One update from a batch (mapping with obs, action, reward, next_obs,
        done) -> (actor loss, or None when this call skipped the actor, critic
        loss).

        The reference draws the smoothing noise in place into the batch's
        action tensor (``actions.data.normal_``), which destroys the sampled
        actions; here the one ``normal_(0, policy_noise)`` draw goes into a
        fresh tensor of the same shape — the same consumption of the device
        generator and the same values — and ``experiences["action"]`` is
        left as it was."""
        obs, actions, rewards, next_obs, dones = batch(self, experiences, "obs", "action", "reward", "next_obs", "done")
        actions = actions.to(torch.float32).reshape(obs.shape[0], self.action_dim)
        rewards = rewards.to(torch.float32).reshape(-1).contiguous()
        dones = dones.to(torch.float32).reshape(-1).contiguous()
        critic_groups = self._groups[1:]
        critics = [getattr(self, g.net) for g in critic_groups]
        targets = [getattr(self, g.target) for g in critic_groups]

        q = [critic(obs, actions) for critic in critics]
        with torch.no_grad():
            next_actions = self.actor_target(next_obs).contiguous()
            noise = torch.empty_like(actions, memory_format=torch.contiguous_format).normal_(0, policy_noise)
            if self._bounds is None or self._bounds[0].device != next_actions.device:
                self._bounds = (self.action_low.to(next_actions.device), self.action_high.to(next_actions.device))
            K.td3_smooth_actions(next_actions, noise, *self._bounds, noise_clip, out=next_actions)
            q_next = [target(next_obs, next_actions) for target in targets]
        twin = len(critics) == 2
        critic_loss = MSECriticLoss.apply(q[0], q[1] if twin else None, q_next[0], q_next[1] if twin else None,
                                          rewards, dones, float(self.gamma), False)
        for g in critic_groups:
            getattr(self, g.opt).zero_grad()
        critic_loss.backward()
        for g in critic_groups:
            self._step(g)

        self.learn_counter += 1
        if self.learn_counter % self.policy_freq != 0:
            return None, critic_loss.item()
        actor_loss = -critics[0](obs, self.actor(obs)).mean()
        self.actor_optimizer.zero_grad()
        actor_loss.backward()
        self._step(_ACTOR)
        for g in self._groups:
            self.soft_update(g)
        return actor_loss.item(), critic_loss.item()

    # ---- evaluation, clones, checkpoints ----------------------------------------
    @torch.no_grad()
    def test(self, env, swap_channels: bool = False, max_steps: int | None = None, loop: int = 3) -> float:
        self.set_training_mode(False)
        fitness = _evaluate(self, env, lambda o: self.get_action(o, training=False), max_steps, loop)
        self.set_training_mode(True)
        return fitness

    def clone(self, index: int | None = None, wrap: bool = True):
        """Deep copy with a new index (EvolvableAlgorithm.clone, core/base.py).
        The copy gets flat buffers of its own for every group whose flat
        state is live here, so its tensors are laid out as this agent's are
        and the two compute the same update from the same batch and seed."""
        flat = self.__dict__.pop("_flat", None) or {}
        try:
            c = super().clone(index, wrap)
        finally:
            if flat:
                self.__dict__["_flat"] = flat
        for g in self._groups:
            fs = flat.get(g.net)
            if fs is not None and fs.valid(*(getattr(self, n) for n in g[:3])):
                flat_state(c, g)
        return c

    # core/base.py:939-1072 layout (checkpoint.py) with the reference's attribute
    # names; ``network_arch`` records what architecture mutations changed, so
    # a freshly built agent can take the weights
    def _ckpt_extra(self, ck: dict) -> None:
        for k in self._CKPT_EXTRA:
            ck[k] = C._plain(getattr(self, k))
        for k in self._CKPT_ARRAYS:
            ck[k] = torch.from_numpy(np.array(getattr(self, k), dtype=np.float64))
        save_arch(self, ck)

    def _ckpt_restore(self, ck: dict) -> None:
        restore_arch(self, ck)
        for k in self._CKPT_EXTRA:
            if k in ck:
                setattr(self, k, ck[k])
        for k in self._CKPT_ARRAYS:
            if k in ck:
                setattr(self, k, ck[k].numpy().copy())

    @classmethod
    def from_init_hp(cls, observation_space, action_space, net_config, INIT_HP, index=0, num_envs=1, device="cuda",
                     **kw):
        """create_population's construction (utils/utils.py:466-493, 560-587).
        ``SHARE_ENCODERS`` defaults to False here (the reference's True is
        outside this path and raises)."""
        return cls(observation_space, action_space, O_U_noise=INIT_HP.get("O_U_NOISE", True),
                   expl_noise=INIT_HP.get("EXPL_NOISE", 0.1), vect_noise_dim=num_envs,
                   mean_noise=INIT_HP.get("MEAN_NOISE", 0.0), theta=INIT_HP.get("THETA", 0.15),
                   dt=INIT_HP.get("DT", 0.01), index=index, net_config=net_config,
                   batch_size=INIT_HP.get("BATCH_SIZE", 64), lr_actor=INIT_HP.get("LR_ACTOR", 0.0001),
                   lr_critic=INIT_HP.get("LR_CRITIC", 0.001), learn_step=INIT_HP.get("LEARN_STEP", 5),
                   gamma=INIT_HP.get("GAMMA", 0.99), tau=INIT_HP.get("TAU", cls._DEFAULT_TAU),
                   policy_freq=INIT_HP.get("POLICY_FREQ", 2), share_encoders=INIT_HP.get("SHARE_ENCODERS", False),
                   device=device, **kw)


class DDPG(_DeterministicPolicyGradient):
    algo = "DDPG"
    _groups = (_ACTOR, NetGroup("critic", "critic_target", "critic_optimizer", "lr_critic"))
    _DEFAULT_TAU = 0.001

    def __init__(self, observation_space, action_space, O_U_noise: bool = True, expl_noise=0.1,
                 vect_noise_dim: int = 1, mean_noise: float = 0.0, theta: float = 0.15, dt: float = 1e-2,
                 index: int = 0, hp_config=None, net_config: dict[str, Any] | None = None, batch_size: int = 64,
                 lr_actor: float = 1e-4, lr_critic: float = 1e-3, learn_step: int = 5, gamma: float = 0.99,
                 tau: float = 1e-3, normalize_images: bool = True, mut=None, policy_freq: int = 2,
                 actor_network=None, critic_network=None, share_encoders: bool = False, device="cuda",
                 accelerator=None, wrap: bool = True) -> None:
        self._setup(observation_space, action_space, O_U_noise, expl_noise, vect_noise_dim, mean_noise, theta, dt,
                    index, hp_config, net_config, batch_size, lr_actor, lr_critic, learn_step, gamma, tau,
                    normalize_images, mut, policy_freq, (actor_network, critic_network), share_encoders, device, wrap)

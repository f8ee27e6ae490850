"""Drop-in ``NeuralUCB`` (agilerl/algorithms/neural_ucb_bandit.py:20-339) and
the base it shares with ``NeuralTS`` (neural_ts_bandit.py): a ``ValueNetwork``
scores every arm of a context, the confidence width of arm k is
gamma sqrt(g_k Sigma^-1 g_k^T) with g_k the gradient of its score with respect
to the exploration layer (the network's output Linear), and Sigma^-1 takes a
Sherman-Morrison update with the chosen arm's gradient.

``get_action``.  The reference builds g with one backward pass per arm, two
batched matmuls, a host argmax and a D x D by D x D product.  The exploration
layer is a ``Linear(H, 1)`` with no activation after it, so g_k is
[h_k, 1] / sqrt(weight.size(0)) with h_k the layer's input, which the
forward pass already has: here the step is one no-grad forward, one
``agx_bandit_select`` (include/agx_bandit.h: widths, scores, masked argmax and
the rank-1 update of Sigma^-1 on the device) and one scalar read-back; from
the second call of an observation shape on, forward and selection are
replayed from a captured graph.  A replay is valid only while the tensors it
baked in are the live ones: every parameter's address, Sigma^-1's, the
Thompson counter's and the exploration layer are compared on every call (the
flat learner state re-points the parameters when it adopts the network; a
mutation, a clone or a checkpoint load replaces them).  ``AGX_LEARN_GRAPH=0``
keeps every call eager.  An exploration layer of another form (an output
activation, no bias, several outputs) takes the reference's per-arm autograd
loop, whose g goes to the same kernel as an explicit matrix.  On the CPU the
same arithmetic runs as torch ops (kernels.bandit_select_torch).

``learn``: MSE(reward, prediction) + reg ||theta_out - theta_0||^2, backward,
Adam without clipping — the flat one-launch Adam (flat_state.py, no target
network) replayed from a captured graph from the second update of a shape on
(learn_graph.py); ``learn_device`` leaves the loss on the device.

Parity notes: theta_0 is a detached copy, so the
regulariser has a gradient (in the reference theta_0 stays attached to the
live parameters and the term's gradient cancels until a checkpoint is
loaded); Sigma^-1 survives mutations under the ``_reinit_bandit_grads`` rule
(hpo/mutation.py) where the reference's mutation hook resets it; NeuralTS
draws its noise from the kernel's own Philox stream.
"""

from __future__ import annotations

import weakref
from typing import Any

import numpy as np
import torch
from torch import nn

from .. import kernels as K
from ..modules.mlp import EvolvableMLP
from ..networks.base import as_config, image_norm_bounds, is_image_space, mlp_net_config
from ..networks.value_networks import ValueNetwork
from . import checkpoint as C
from . import learn_graph
from .ddpg import restore_arch, save_arch
from .dqn import _net_kwargs, _obs_tensor
from .evolvable import EvolvableAgentMixin, NetGroup
from .flat_state import flat_state
from .offpolicy import batch

_U64 = (1 << 64) - 1
# agent -> {"sig": what the graphs baked in, "table": {key: _ActGraph}}; weak, so never deep-copied with the agent
_ACT_GRAPHS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


class _ActGraph:
    __slots__ = ("eager", "graph", "obs", "mask", "out", "failed")

    def __init__(self):
        self.eager, self.graph, self.obs, self.mask, self.out, self.failed = 0, None, None, None, None, False


class _NeuralBandit(EvolvableAgentMixin, C.TorchCheckpointMixin):
    """What NeuralUCB and NeuralTS share: everything but the score's noise."""

    _groups = (NetGroup("actor", None, "optimizer", "lr"),)  # no target network
    _thompson = False
    #: attributes beyond checkpoint.HP_NAMES that a checkpoint carries
    _CKPT_EXTRA = ("lamb", "reg", "numel", "regret", "noise_base")

    def _setup(self, observation_space, action_space, index, hp_config, net_config, gamma, lamb, reg, batch_size,
               normalize_images, lr, learn_step, mut, actor_network, device, wrap) -> None:
        assert learn_step >= 1, "Learn step must be greater than or equal to one."
        assert isinstance(learn_step, int), "Learn step rate must be an integer."
        assert isinstance(gamma, (float, int)), "Scaling factor must be a float or integer."
        assert gamma > 0, "Scaling factor must be positive."
        assert isinstance(lamb, (float, int)), "Regularization parameter lambda must be a float or integer."
        assert lamb > 0, "Regularization parameter lambda must be greater than zero."
        assert isinstance(reg, float), "Loss regularization parameter must be a float."
        assert reg > 0, "Loss regularization parameter must be greater than zero."
        assert isinstance(batch_size, int), "Batch size must be an integer."
        assert batch_size >= 1, "Batch size must be greater than or equal to one."
        assert isinstance(lr, float), "Learning rate must be a float."
        assert lr > 0, "Learning rate must be greater than zero."
        assert isinstance(wrap, bool), "Wrap models flag must be boolean value True or False."
        if not hasattr(action_space, "n"):
            raise NotImplementedError(f"agx {self.algo} takes a Discrete action space (one action per arm)")
        if actor_network is not None:
            raise NotImplementedError("custom actor modules: use net_config networks")
        self.observation_space, self.action_space = observation_space, action_space
        self.index, self.net_config, self.mut = index, net_config, mut
        self.gamma, self.lamb, self.reg = gamma, lamb, reg
        self.batch_size, self.lr, self.learn_step = batch_size, lr, learn_step
        self.device = torch.device(device)
        self.action_dim = int(action_space.n)
        self.obs_dim = int(np.prod(observation_space.shape))
        cfg = _net_kwargs(net_config)
        if cfg.get("simba") or cfg.get("recurrent"):
            raise NotImplementedError("SimBa and recurrent encoders are outside the agx path")
        self._image = is_image_space(observation_space)
        if not hasattr(observation_space, "spaces"):  # neural_ucb_bandit.py:141-146: no LayerNorm
            enc = as_config(cfg.get("encoder_config"))
            if enc is None and not self._image:
                enc = mlp_net_config([64, 64], output_activation="ReLU", output_vanish=False)
            if enc is not None:
                enc["layer_norm"] = False
                cfg["encoder_config"] = enc
        self.actor = ValueNetwork(observation_space, device=self.device, **cfg)
        self.normalize_images = normalize_images
        self._img_norm = image_norm_bounds(observation_space) if self._image and normalize_images else None
        self.actor.set_image_norm(self._img_norm)
        self.optimizer = torch.optim.Adam(self.actor.parameters(), lr=lr)
        self.actor.init_weights_gaussian(std_coeff=4, output_coeff=2)
        self.init_params()
        self._init_registry(hp_config)
        self.regret: list = [0]
        self.scores: list[float] = []
        self.fitness: list[float] = []
        self.steps: list[int] = [0]
        # the Thompson stream: key = noise_base mixed with the agent's index (a clone
        # with a new index draws its own noise), counter advanced by the kernel
        self.noise_base = int(torch.initial_seed()) & _U64
        self.ts_counter = torch.zeros(1, dtype=torch.int64, device=self.device)

    @classmethod
    def from_init_hp(cls, observation_space, action_space, net_config, INIT_HP, index=0, device="cuda", **kw):
        """The INIT_HP keys create_population reads (utils/utils.py:682-722)."""
        return cls(observation_space, action_space, index=index, net_config=net_config,
                   gamma=INIT_HP.get("GAMMA", 1), lamb=INIT_HP.get("LAMBDA", 1), reg=INIT_HP.get("REG", 0.000625),
                   batch_size=INIT_HP.get("BATCH_SIZE", 64), lr=INIT_HP.get("LR", cls._DEFAULT_LR),
                   learn_step=INIT_HP.get("LEARN_STEP", 2), device=device, **kw)

    # ---- the exploration layer -----------------------------------------------------------
    def _theta(self) -> torch.Tensor:
        return torch.cat([w.flatten() for w in self.exp_layer.parameters() if w.requires_grad])

    def _read_exp_layer(self) -> None:
        self.exp_layer = self.actor.get_output_dense()
        self.numel = sum(w.numel() for w in self.exp_layer.parameters() if w.requires_grad)
        self.theta_0 = self._theta().detach().clone()

    def init_params(self) -> None:
        """neural_ucb_bandit.py:173-183."""
        self._read_exp_layer()
        self.sigma_inv = self.lamb * torch.eye(self.numel, dtype=torch.float32, device=self.device)

    def _exp_sizes(self) -> dict:
        return {k: p.numel() for k, p in self.exp_layer.named_parameters() if p.requires_grad}

    def _reinit_bandit_grads(self, old_sizes: dict) -> None:
        """After an architecture mutation: exp_layer, numel and theta_0 re-read,
        Sigma^-1 carried over by hpo.mutation.reinit_bandit_grads."""
        self._read_exp_layer()
        from ..hpo.mutation import reinit_bandit_grads

        new = reinit_bandit_grads(self.sigma_inv.cpu().numpy(), old_sizes, self._exp_sizes(), float(self.lamb))
        self.sigma_inv = torch.from_numpy(np.ascontiguousarray(new, dtype=np.float32)).to(self.device)

    def architecture_mutation(self, new_layer_prob: float, rng) -> str:
        old = self._exp_sizes()
        applied = super().architecture_mutation(new_layer_prob, rng)
        self._reinit_bandit_grads(old)
        return applied

    def mutation_hook(self) -> None:
        """After any mutation the exploration layer may be a new module
        (recreated networks) and theta_0 is re-read, as the reference's hook
        (init_params) does; Sigma^-1 is kept unless its size no longer fits."""
        self._read_exp_layer()
        if self.sigma_inv.shape[0] != self.numel:
            self.sigma_inv = self.lamb * torch.eye(self.numel, dtype=torch.float32, device=self.device)

    def closed_form(self) -> bool:
        """Whether g_k = [h_k, 1] / sqrt(weight.size(0)) holds: the exploration
        layer a plain Linear with a bias and one output, nothing but the
        identity after it."""
        layer = self.exp_layer
        if type(layer) is not nn.Linear or layer.bias is None or layer.out_features != 1:
            return False
        if not (layer.weight.requires_grad and layer.bias.requires_grad):
            return False
        after = list(self.actor.head_net.model.children())
        if not any(m is layer for m in after):
            return False
        after = after[[m is layer for m in after].index(True) + 1:]
        return all(isinstance(m, nn.Identity) for m in after)

    @property
    def _scale(self) -> float:
        return float(1.0 / np.sqrt(self.exp_layer.weight.size(0)))

    @property
    def noise_seed(self) -> int:
        return (self.noise_base + 0x9E3779B97F4A7C15 * (int(self.index) + 1)) & _U64

    def _obs(self, obs) -> torch.Tensor:
        return _obs_tensor(self, obs)

    # ---- get_action ------------------------------------------------------------------------
    def arm_gradients(self, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """(mu [A], g [A, numel]) by the reference's per-arm backward passes
        (neural_ucb_bandit.py:204-235)."""
        mu_raw = self.actor(x).reshape(-1)
        single = mu_raw.numel() == 1 and self.action_dim > 1
        rows = 1 if single else mu_raw.numel()
        g = torch.zeros((self.action_dim if single else rows, self.numel), device=self.device)
        for k in range(rows):
            self.optimizer.zero_grad()
            mu_raw[k].backward(retain_graph=True)
            g[k] = torch.cat([w.grad.detach().flatten() / np.sqrt(self.exp_layer.weight.size(0))
                              for w in self.exp_layer.parameters() if w.requires_grad])
        if single:
            g[:] = g[0].clone()
        mu = mu_raw.repeat(self.action_dim) if single else mu_raw
        return mu.detach(), g

    @torch.no_grad()
    def arm_features(self, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """(mu [A], h [A, H]) of one forward: h is the exploration layer's
        input; a single-row context is repeated over the arms."""
        out, h = self.actor.forward_with_features(x)
        mu = out.reshape(-1)
        if mu.numel() == 1 and self.action_dim > 1:
            mu, h = mu.repeat(self.action_dim), h.reshape(1, -1).repeat(self.action_dim, 1)
        return mu, h.reshape(mu.numel(), -1)

    def _select(self, x: torch.Tensor, mask) -> torch.Tensor:
        """Forward + selection on ``x`` -> the action, on the device."""
        select = K.bandit_select if self.device.type == "cuda" else K.bandit_select_torch
        if self.closed_form():
            mu, h = self.arm_features(x)
            bias_one, scale = True, self._scale
        else:
            mu, h = self.arm_gradients(x)
            bias_one, scale = False, 1.0
        action, scores, quad = select(h if h.stride(-1) == 1 else h.contiguous(), mu.contiguous(), self.sigma_inv,
                                      mask, bias_one=bias_one, scale=scale, gamma=float(self.gamma),
                                      thompson=self._thompson, seed=self.noise_seed, counter=self.ts_counter)
        self.last_scores, self.last_quad = scores, quad
        return action

    def _graph_signature(self) -> tuple:
        return (tuple(p.data_ptr() for p in self.actor.parameters()), self.sigma_inv.data_ptr(),
                self.ts_counter.data_ptr(), id(self.exp_layer), int(self.exp_layer.in_features), self.actor.training)

    def _replayed(self, x: torch.Tensor, mask):
        """The action from the captured graph of this observation shape, or
        None: the caller runs the step eagerly (the first call of a shape, a
        capture that failed, graphs disabled, hooks on the network)."""
        if (not learn_graph.enabled() or not self.closed_form() or torch.cuda.is_current_stream_capturing()
                or learn_graph._hooked(self.actor)):
            return None
        slot = _ACT_GRAPHS.get(self)
        sig = self._graph_signature()
        if slot is None or slot["sig"] != sig:  # a stale graph is never replayed: dropped with everything it holds
            slot = _ACT_GRAPHS[self] = {"sig": sig, "table": {}}
        key = (tuple(x.shape), x.dtype, mask is not None, float(self.gamma), self.noise_seed, self._scale)
        ent = slot["table"].get(key)
        if ent is None:
            ent = slot["table"][key] = _ActGraph()
        if ent.graph is None:
            if ent.failed or ent.eager < 1:
                ent.eager += 1
                return None
            ent.obs, ent.mask = x.clone(), None if mask is None else mask.clone()
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            try:
                with torch.cuda.graph(graph):
                    ent.out = (self._select(ent.obs, ent.mask), self.last_scores, self.last_quad)
            except Exception as exc:  # noqa: BLE001 - any capture failure: this shape stays eager
                import warnings

                warnings.warn(f"agx bandit graph: capture failed ({exc!r}); get_action stays eager for this shape")
                ent.failed, ent.obs, ent.mask, ent.out = True, None, None, None
                torch.cuda.synchronize()
                return None
            ent.graph = graph
        else:
            ent.obs.copy_(x)
            if mask is not None:
                ent.mask.copy_(mask)
        ent.graph.replay()
        action, self.last_scores, self.last_quad = ent.out
        return action

    def get_action(self, obs, action_mask=None, *args: Any, **kwargs: Any) -> int:
        """The arm to pull (neural_ucb_bandit.py:185-259); Sigma^-1 takes the
        chosen arm's update.  ``action_mask``: 1 = legal."""
        x = self._obs(obs)
        mask = None
        if action_mask is not None:
            mask = torch.as_tensor(np.asarray(action_mask).reshape(-1) == 1).to(torch.uint8).to(self.device)
        action = self._replayed(x, mask) if self.device.type == "cuda" else None
        if action is None:
            action = self._select(x, mask)
        return int(action.item())

    # ---- learn -------------------------------------------------------------------------------
    def _loss(self, xs: list) -> torch.Tensor:
        """neural_ucb_bandit.py:273-295 over xs = [obs, reward], and the backward pass."""
        obs, rewards = xs
        pred = self.actor(obs)
        loss = torch.nn.functional.mse_loss(rewards, pred)
        loss = loss + self.reg * torch.norm(self._theta() - self.theta_0) ** 2
        self.optimizer.zero_grad()
        loss.backward()
        return loss.detach()

    def learn_device(self, experiences) -> torch.Tensor:
        """One update; -> the loss as a device scalar, not read back (after a
        replayed update the graph's static output: read it before the next
        update).  ``experiences``: a mapping with ``obs`` and ``reward``, or
        the (obs, reward) pair."""
        if isinstance(experiences, (tuple, list)):
            experiences = dict(zip(("obs", "reward"), experiences))
        xs = batch(self, experiences, "obs", "reward")
        xs[1] = xs[1].to(torch.float32).reshape(xs[0].shape[0], 1)
        fs = flat_state(self)
        nets = (self.actor,)
        g = self.optimizer.param_groups[0]
        key = ("bandit", float(self.reg), tuple(g["betas"]), float(g["eps"]), self.theta_0.data_ptr())
        loss = learn_graph.run(fs, key, xs, self._loss, nets, 0.0, 0.0)
        if loss is None:
            loss = self._loss(xs)
            flat_ok = fs is not None and fs.step(0.0)  # Adam, no clipping: one launch (flat_state.py)
            if not flat_ok:
                self.optimizer.step()
            learn_graph.note_eager(fs, key, xs, nets, flat_ok)
        return loss

    def learn(self, experiences) -> float:
        return float(self.learn_device(experiences).item())

    # ---- evaluation --------------------------------------------------------------------------
    @torch.no_grad()
    def test(self, env, swap_channels: bool = False, max_steps: int = 100, loop: int = 1) -> float:
        """Mean score of ``loop`` passes of ``max_steps`` greedy pulls (the arm
        with the largest predicted reward; neural_ucb_bandit.py:301-339)."""
        training = self.actor.training
        self.actor.eval()
        rewards = []
        for _ in range(loop):
            obs = env.reset()
            score = 0.0
            for _ in range(max_steps):
                if swap_channels:
                    obs = np.moveaxis(np.asarray(obs), -1, -3)
                action = int(torch.argmax(self.actor(self._obs(obs)).reshape(-1)).item())
                obs, reward = env.step(action)
                score += float(reward)
            rewards.append(score)
        self.actor.train(training)
        fit = float(np.mean(rewards))
        self.fitness.append(fit)
        return fit

    # ---- checkpoints ---------------------------------------------------------------------------
    def _ckpt_extra(self, ck: dict) -> None:
        for k in self._CKPT_EXTRA:
            ck[k] = C._plain(getattr(self, k))
        ck["sigma_inv"], ck["theta_0"] = C._plain(self.sigma_inv), C._plain(self.theta_0)
        ck["ts_counter"] = int(self.ts_counter.item())
        if isinstance(getattr(self.actor, "encoder", None), EvolvableMLP):
            save_arch(self, ck)
            ck["network_activation"] = self.actor.activation

    def _into(self, name: str, value: torch.Tensor) -> None:
        """A loaded tensor into the live one where the shape allows (captured
        graphs hold its address), else in its place."""
        cur = getattr(self, name)
        value = value.to(device=self.device, dtype=cur.dtype)
        if cur.shape == value.shape:
            cur.copy_(value)
        else:
            setattr(self, name, value.clone())

    def _ckpt_restore(self, ck: dict) -> None:
        if "network_arch" in ck:
            act = ck.get("network_activation")
            if act and self.actor.activation != act:
                self.actor.change_activation(act, output=False)
            restore_arch(self, ck)
        for k in self._CKPT_EXTRA:
            if k in ck:
                setattr(self, k, ck[k])
        self._read_exp_layer()  # theta_0 is overwritten below; the state dict is loaded after this hook
        if self.sigma_inv.shape[0] != self.numel:
            self.sigma_inv = self.lamb * torch.eye(self.numel, dtype=torch.float32, device=self.device)
        with torch.no_grad():
            if "sigma_inv" in ck:
                self._into("sigma_inv", ck["sigma_inv"])
            if "theta_0" in ck:
                self._into("theta_0", ck["theta_0"])
            if "ts_counter" in ck:
                self.ts_counter.fill_(int(ck["ts_counter"]))


class NeuralUCB(_NeuralBandit):
    algo = "NeuralUCB"
    _DEFAULT_LR = 1e-3

    def __init__(self, observation_space, action_space, index: int = 0, hp_config=None, net_config=None,
                 gamma: float = 1.0, lamb: float = 1.0, reg: float = 0.000625, batch_size: int = 64,
                 normalize_images: bool = True, lr: float = 1e-3, learn_step: int = 2, mut=None,
                 actor_network=None, device="cpu", accelerator=None, wrap: bool = True):
        self._setup(observation_space, action_space, index, hp_config, net_config, gamma, lamb, reg, batch_size,
                    normalize_images, lr, learn_step, mut, actor_network, device, wrap)

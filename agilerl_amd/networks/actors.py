"""``DeterministicActor`` (agilerl/networks/actors.py:49-230): EvolvableMLP
encoder + head named "actor"; output activation GumbelSoftmax for Discrete
action spaces, Tanh for Box (or a user choice among the allowed ones)."""

from __future__ import annotations

import warnings

import torch

from .base import EvolvableNetwork, as_config, flatdim, mlp_net_config

_ALLOWED = ("Tanh", "Softsign", "Sigmoid", "Softmax", "GumbelSoftmax")


def get_output_bounds(output_activation: str):
    if output_activation in ("Tanh", "Softsign"):
        return -1.0, 1.0
    if output_activation in ("Sigmoid", "Softmax", "GumbelSoftmax"):
        return 0.0, 1.0
    return None, None


class DeterministicActor(EvolvableNetwork):
    def __init__(self, observation_space, action_space, encoder_cls=None, encoder_config=None, head_config=None,
                 min_latent_dim: int = 8, max_latent_dim: int = 128, latent_dim: int = 32, simba: bool = False,
                 recurrent: bool = False, device="cpu", random_seed: int | None = None,
                 encoder_name: str = "encoder") -> None:
        super().__init__(observation_space, encoder_cls=encoder_cls, encoder_config=encoder_config,
                         action_space=action_space, min_latent_dim=min_latent_dim, max_latent_dim=max_latent_dim,
                         latent_dim=latent_dim, simba=simba, recurrent=recurrent, device=device,
                         random_seed=random_seed, encoder_name=encoder_name)
        discrete = hasattr(action_space, "n")
        if discrete:
            self.action_low = self.action_high = None
            output_activation = "GumbelSoftmax"
        else:
            self.action_low = torch.as_tensor(action_space.low, dtype=torch.float32)
            self.action_high = torch.as_tensor(action_space.high, dtype=torch.float32)
            output_activation = "Tanh"
        head_config = as_config(head_config)
        if head_config is not None and "output_activation" in head_config:
            user = head_config["output_activation"]
            if user in _ALLOWED:
                output_activation = user
            else:
                warnings.warn(f"Output activation must be one of the following: {', '.join(_ALLOWED)}. Got {user} "
                              "instead. Using default output activation.", stacklevel=2)
        self.output_activation = output_activation
        if head_config is None:
            head_config = mlp_net_config([32], output_activation=output_activation)
        else:
            head_config["output_activation"] = output_activation
        self.output_size = flatdim(action_space)
        self.head_net = self.create_mlp(self.latent_dim, self.output_size, "actor", head_config)

    @staticmethod
    def rescale_action(action: torch.Tensor, low: torch.Tensor, high: torch.Tensor,
                       output_activation: str) -> torch.Tensor:
        """[min_out, max_out] -> [low, high] (actors.py:153-188)."""
        lo, hi = get_output_bounds(output_activation)
        if lo is None or hi is None or low.isinf().any() or high.isinf().any():
            return action
        return (low + (high - low) * ((action - lo) / (hi - lo))).to(low.dtype)

    def forward(self, obs: torch.Tensor, hidden_state=None):
        if self.recurrent:  # -> (action, next hidden state)
            latent, hidden_state = self.extract_features(obs, hidden_state=hidden_state)
            return self.head_net(latent), hidden_state
        return self.head_net(self.extract_features(obs))


class EvolvableDistribution(torch.nn.Module):
    """The head of a ``StochasticActor`` (agilerl/networks/distributions.py:110-342) for Discrete, Box,
    MultiDiscrete and MultiBinary action spaces: the MLP as ``_wrapped`` and, for Box, the learned ``log_std``
    [1, A] (the reference's state-dict names).  ``forward`` keeps the masked logits for ``log_prob``; sampling
    is torch ops.  ``discrete`` is every space but Box; ``nvec`` (MultiDiscrete) / ``binary`` (MultiBinary) name the two factored heads: K
    categoricals over slices of the logits (actions [.., K]) and n Bernoullis (actions [.., n] of 0 / 1)."""

    def __init__(self, action_space, network, action_std_init: float = 0.0, device="cpu") -> None:
        super().__init__()
        self._wrapped, self.action_space, self.device = network, action_space, device
        self.nvec = [int(n) for n in action_space.nvec] if hasattr(action_space, "nvec") else None
        self.binary = type(action_space).__name__ == "MultiBinary"
        self.discrete = hasattr(action_space, "n") or self.nvec is not None  # a head of logits: no log_std
        self.logits = None
        if not self.discrete:
            self.log_std = torch.nn.Parameter(torch.ones(1, flatdim(action_space), device=device) * action_std_init)

    @property
    def net_config(self):
        return self._wrapped.net_config

    def __deepcopy__(self, memo):
        """A copy without the last forward's logits (a graph tensor cannot be deep-copied)."""
        import copy

        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update(copy.deepcopy({**self.__dict__, "logits": None}, memo))
        return new

    def log_prob(self, action: torch.Tensor) -> torch.Tensor:
        from ..population.nets import bernoulli_head, categorical, gaussian, multi_categorical

        if self.logits is None:
            raise ValueError("Distribution not initialized. Call forward first.")
        if self.nvec is not None:
            return multi_categorical(self.logits, self.nvec, action.long().reshape(-1, len(self.nvec)))[0]
        if self.binary:
            return bernoulli_head(self.logits, action.reshape(self.logits.shape))[0]
        if self.discrete:
            return categorical(self.logits)[0].gather(-1, action.long().reshape(-1, 1)).squeeze(-1)
        return gaussian(self.logits, self.log_std, action)[0]

    def forward(self, latent: torch.Tensor, action_mask=None, sample: bool = True):
        """-> (action, log_prob, entropy); action and log_prob are None without ``sample``."""
        from ..population.nets import bernoulli_head, categorical, gaussian, multi_categorical

        logits = self._wrapped(latent)
        if action_mask is not None:  # distributions.py:16-28: illegal logits -> -1e8
            mask = torch.as_tensor(action_mask, device=logits.device).bool().view(logits.shape)
            logits = torch.where(mask, logits, torch.full_like(logits, -1e8))
        self.logits = logits
        if self.nvec is not None:
            parts = logits.split(self.nvec, dim=-1)
            first = torch.zeros(*logits.shape[:-1], len(self.nvec), dtype=torch.long, device=logits.device)
            entropy = multi_categorical(logits, self.nvec, first)[1]
            action = torch.stack([torch.multinomial(torch.softmax(p, dim=-1), 1).squeeze(-1) for p in parts],
                                 -1) if sample else None
        elif self.binary:
            entropy = bernoulli_head(logits, logits)[1]
            action = torch.bernoulli(torch.sigmoid(logits)) if sample else None
        elif self.discrete:
            entropy = categorical(logits)[1]
            action = torch.multinomial(torch.softmax(logits, dim=-1), 1).squeeze(-1) if sample else None
        else:
            entropy = gaussian(logits, self.log_std, logits)[1]
            action = logits + torch.exp(self.log_std) * torch.randn_like(logits) if sample else None
        return action, (self.log_prob(action) if sample else None), entropy


class StochasticActor(EvolvableNetwork):
    """``StochasticActor`` (agilerl/networks/actors.py:214-425) over Discrete (categorical logits), 1-D Box
    (mean, learned log_std), 1-D MultiDiscrete (sum nvec logits, one categorical per component) and 1-D
    MultiBinary (one Bernoulli logit per bit) action spaces, for recurrent PPO: an encoder, the MLP head "actor"
    and its distribution.  ``squash_output`` is not supported."""

    def __init__(self, observation_space, action_space, encoder_cls=None, encoder_config=None, head_config=None,
                 action_std_init: float = 0.0, squash_output: bool = False, min_latent_dim: int = 8,
                 max_latent_dim: int = 128, latent_dim: int = 32, simba: bool = False, recurrent: bool = False,
                 device="cpu", random_seed: int | None = None, encoder_name: str = "encoder") -> None:
        super().__init__(observation_space, encoder_cls=encoder_cls, encoder_config=encoder_config,
                         action_space=action_space, min_latent_dim=min_latent_dim, max_latent_dim=max_latent_dim,
                         latent_dim=latent_dim, simba=simba, recurrent=recurrent, device=device,
                         random_seed=random_seed, encoder_name=encoder_name)
        if squash_output:
            raise NotImplementedError("agx StochasticActor: squash_output=True is not supported")
        multi, binary = hasattr(action_space, "nvec"), type(action_space).__name__ == "MultiBinary"
        if (multi or binary or not hasattr(action_space, "n")) and (
                len(action_space.shape) != 1 or not (multi or binary or hasattr(action_space, "low"))):
            raise NotImplementedError("agx StochasticActor: Discrete and 1-D Box, MultiDiscrete and MultiBinary "
                                      "action spaces")
        head_config = as_config(head_config)
        if head_config is None:
            head_config = mlp_net_config([32], output_activation=None)
        else:
            head_config["output_activation"] = None
        self.action_std_init, self.squash_output, self.output_activation = action_std_init, False, None
        self.output_size = int(sum(action_space.nvec)) if multi else flatdim(action_space)
        self.head_net = EvolvableDistribution(action_space,
                                              self.create_mlp(self.latent_dim, self.output_size, "actor", head_config),
                                              action_std_init=action_std_init, device=device)

    def action_log_prob(self, action: torch.Tensor) -> torch.Tensor:
        return self.head_net.log_prob(action)

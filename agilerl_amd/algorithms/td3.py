"""Drop-in ``TD3`` (agilerl/algorithms/td3.py:30-616) for Box observations
(vectors) and Box actions: twin critics, target-policy smoothing, delayed
actor and target updates.

The update is the shared one of algorithms/ddpg.py with two critics: the
smoothing is one ``agx_td3_smooth_actions`` launch, the twin-critic target
y = r + (1 - d) gamma min(Q1'(s', a'), Q2'(s', a')), MSE(Q1, y) + MSE(Q2, y)
and both gradients one ``agx_td3_critic_target`` launch, and each of the
three Adam steps and three soft updates one launch over the network's flat
buffers (include/agx_td3.h, flat_state.py).
"""

from __future__ import annotations

from typing import Any

from .ddpg import _ACTOR, _DeterministicPolicyGradient
from .evolvable import NetGroup


class TD3(_DeterministicPolicyGradient):
    algo = "TD3"
    # lr_critic drives both critic optimizers (reinit_optimizers re-makes the two)
    _groups = (_ACTOR, NetGroup("critic_1", "critic_target_1", "critic_1_optimizer", "lr_critic"),
               NetGroup("critic_2", "critic_target_2", "critic_2_optimizer", "lr_critic"))
    _DEFAULT_TAU = 0.005

    def __init__(self, observation_space, action_space, O_U_noise: bool = True, vect_noise_dim: int = 1,
                 expl_noise=0.1, mean_noise: float = 0.0, theta: float = 0.15, dt: float = 1e-2, index: int = 0,
                 hp_config=None, net_config: dict[str, Any] | None = None, batch_size: int = 64,
                 lr_actor: float = 1e-4, lr_critic: float = 1e-3, learn_step: int = 5, gamma: float = 0.99,
                 tau: float = 0.005, normalize_images: bool = True, mut=None, policy_freq: int = 2,
                 actor_network=None, critic_networks=None, share_encoders: bool = False, device="cuda",
                 accelerator=None, wrap: bool = True) -> None:
        self._setup(observation_space, action_space, O_U_noise, expl_noise, vect_noise_dim, mean_noise, theta, dt,
                    index, hp_config, net_config, batch_size, lr_actor, lr_critic, learn_step, gamma, tau,
                    normalize_images, mut, policy_freq, (actor_network, critic_networks), share_encoders, device,
                    wrap)

"""Drop-in ``NeuralTS`` (agilerl/algorithms/neural_ts_bandit.py:20-336):
NeuralUCB's network, update and covariance (neural_ucb_bandit.py here) with a
Thompson-sampled score, score_k ~ N(mu_k, (gamma sqrt(g_k Sigma^-1 g_k^T))^2).

The reference draws the normals with ``torch.normal`` on the global
generator.  Here ``agx_bandit_select`` draws them on the device: z_k is the
Box-Muller normal of the Philox4x32-10 block of (the agent's noise seed, its
call counter, arm k) (include/agx_bandit.h), so the whole step stays one
launch and a replayed graph draws fresh noise on every replay (the counter
lives in device memory and the kernel advances it).  The distribution is the
reference's; the stream is not.  The noise seed mixes
``torch.initial_seed()`` at construction with the agent's index; a clone
keeps the counter and, with a new index, draws its own noise.
"""

from __future__ import annotations

from .neural_ucb_bandit import _NeuralBandit


class NeuralTS(_NeuralBandit):
    algo = "NeuralTS"
    _thompson = True
    _DEFAULT_LR = 3e-3

    def __init__(self, observation_space, action_space, index: int = 0, hp_config=None, net_config=None,
                 gamma: float = 1.0, lamb: float = 1.0, reg: float = 0.000625, batch_size: int = 64,
                 lr: float = 3e-3, normalize_images: bool = True, learn_step: int = 2, mut=None,
                 actor_network=None, device="cpu", accelerator=None, wrap: bool = True):
        self._setup(observation_space, action_space, index, hp_config, net_config, gamma, lamb, reg, batch_size,
                    normalize_images, lr, learn_step, mut, actor_network, device, wrap)

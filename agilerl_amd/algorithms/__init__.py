"""Drop-in algorithm classes (agilerl.algorithms) on the agx hot path."""

from .cqn import CQN
from .ddpg import DDPG
from .dqn import DQN, RainbowDQN
from .ippo import IPPO
from .maddpg import MADDPG
from .matd3 import MATD3
from .neural_ts_bandit import NeuralTS
from .neural_ucb_bandit import NeuralUCB
from .ppo import PPO
from .td3 import TD3

__all__ = ["PPO", "DQN", "RainbowDQN", "MADDPG", "MATD3", "DDPG", "TD3", "CQN", "NeuralUCB", "NeuralTS",
           "IPPO"]

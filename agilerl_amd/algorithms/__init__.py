"""Drop-in algorithm classes (agilerl.algorithms) on the agx hot path."""

from .ddpg import DDPG
from .dqn import DQN, RainbowDQN
from .maddpg import MADDPG
from .ppo import PPO
from .td3 import TD3

__all__ = ["PPO", "DQN", "RainbowDQN", "MADDPG", "DDPG", "TD3"]

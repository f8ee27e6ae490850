from .actors import DeterministicActor
from .base import EvolvableNetwork
from .q_networks import ContinuousQNetwork, DuelingDistributionalMLP, QNetwork, RainbowQNetwork
from .value_networks import ValueNetwork

__all__ = ["EvolvableNetwork", "QNetwork", "RainbowQNetwork", "DuelingDistributionalMLP", "ContinuousQNetwork",
           "DeterministicActor", "ValueNetwork"]

"""``ValueNetwork`` (agilerl/networks/value_networks.py:12-129): an encoder and
a "value" head with one output — the network of the neural bandits, whose
output ``Linear(H, 1)`` is their exploration layer.  Same module tree and
state-dict keys as the reference (``encoder.model.encoder_linear_layer_1.
weight``, ``head_net.model.value_linear_layer_output.weight`` ...).  MLP and
CNN encoders; SimBa and recurrent encoders raise, as for every network here.
"""

from __future__ import annotations

import torch
from torch import nn

from ..modules.mlp import EvolvableMLP
from .base import EvolvableNetwork, as_config, mlp_net_config


class ValueNetwork(EvolvableNetwork):
    def __init__(self, observation_space, encoder_cls=None, encoder_config=None, head_config=None,
                 min_latent_dim: int = 8, max_latent_dim: int = 128, latent_dim: int = 32, simba: bool = False,
                 recurrent: bool = False, device="cpu", random_seed: int | None = None,
                 encoder_name: str = "encoder") -> None:
        super().__init__(observation_space, encoder_cls=encoder_cls, encoder_config=encoder_config, action_space=None,
                         min_latent_dim=min_latent_dim, max_latent_dim=max_latent_dim, latent_dim=latent_dim,
                         simba=simba, recurrent=recurrent, device=device, random_seed=random_seed,
                         encoder_name=encoder_name)
        head_config = as_config(head_config)
        if head_config is None:
            head_config = mlp_net_config([32], output_activation=None)
        self.head_net = self.create_mlp(self.latent_dim, 1, "value", head_config)

    def forward(self, x: torch.Tensor, hidden_state=None) -> torch.Tensor:
        return self.head_net(self.extract_features(x))

    def get_output_dense(self) -> nn.Module:
        return self.head_net.get_output_dense()

    def init_weights_gaussian(self, std_coeff: float = 4, output_coeff: float = 4) -> None:
        """EvolvableNetwork.init_weights_gaussian (networks/base.py:390-412),
        draw for draw: the encoder with ``std_coeff`` (its own output layer
        with the module's default coefficient), then the head with
        ``std_coeff`` and its output layer with ``output_coeff``.  A CNN
        encoder keeps its initialisation."""
        if isinstance(self.encoder, EvolvableMLP):
            self.encoder.init_weights_gaussian(std_coeff=std_coeff)
        self.head_net.init_weights_gaussian(std_coeff=std_coeff, output_coeff=output_coeff)

    def forward_with_features(self, x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """-> (the output, the input of the output layer): the head's layers
        called one by one up to ``get_output_dense()``, no module hook.  Only
        meaningful when nothing follows that layer but the identity."""
        out = self.extract_features(x)
        dense = self.get_output_dense()
        h = None
        for layer in self.head_net.model.children():
            if layer is dense:
                h = out
            out = layer(out)
        return out, h

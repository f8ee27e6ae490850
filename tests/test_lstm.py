"""EvolvableLSTM (modules/lstm.py) and the recurrent network layer on the CPU: the reference's weights under a
seed, its mutations and its hidden-state plumbing."""

import pytest
import torch
from agilerl_amd.envs import Box
from torch import nn

from agilerl_amd.modules.lstm import EvolvableLSTM
from agilerl_amd.networks.actors import DeterministicActor
from agilerl_amd.networks.value_networks import ValueNetwork


def test_seeded_state_dict_is_the_reference_order():
    torch.manual_seed(3)
    got = EvolvableLSTM(5, 32, 7, num_layers=2, name="enc").state_dict()
    torch.manual_seed(3)
    lstm, lin = nn.LSTM(5, 32, 2, batch_first=True), nn.Linear(32, 7)
    want = {**{f"model.enc_lstm.{k}": v for k, v in lstm.state_dict().items()},
            **{f"model.enc_lstm_output.{k}": v for k, v in lin.state_dict().items()}}
    assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in want)


def test_mutations_stay_in_bounds_and_keep_parameters():
    m = EvolvableLSTM(5, 32, 7, min_hidden_state_size=32, max_hidden_state_size=64, max_layers=2, random_seed=0)
    w = m.lstm.weight_hh_l0.detach().clone()
    assert m.add_node(32) == {"numb_new_nodes": 32} and m.hidden_state_size == 64
    assert torch.equal(m.lstm.weight_hh_l0[:32, :32], w[:32, :32])
    m.add_node(16)
    assert m.hidden_state_size == 64  # at the maximum
    m.remove_node(32)
    m.remove_node(16)
    assert m.hidden_state_size == 32  # at the minimum
    assert m.add_layer() is None and m.num_layers == 2 and m.lstm.num_layers == 2
    assert "numb_new_nodes" in m.add_layer() and m.num_layers == 2 and m.last_mutation_attr == "add_node"
    assert m.remove_layer() is None and m.num_layers == 1
    m.change_activation("Tanh")
    assert isinstance(m.model["lstm_output_activation"], nn.Tanh) and m.net_config["output_activation"] == "Tanh"


@pytest.mark.parametrize("make", [lambda s: ValueNetwork(s, recurrent=True, latent_dim=16),
                                  lambda s: DeterministicActor(s, Box(-1.0, 1.0, (2,)), recurrent=True)],
                         ids=["value", "actor"])
def test_recurrent_network_step_and_sequence(make):
    net = make(Box(-1.0, 1.0, (6,)))
    hid = net.initialize_hidden_state(5)
    assert {k: tuple(v.shape) for k, v in hid.items()} == {"encoder_h": (1, 5, 128), "encoder_c": (1, 5, 128)}
    out, hid = net(torch.randn(5, 6), hid)
    seq, hid2 = net(torch.randn(5 * 4, 6), hid)
    assert out.shape[0] == 5 and seq.shape[0] == 20 and hid2["encoder_h"].shape == (1, 5, 128)
    assert not torch.equal(hid2["encoder_c"], hid["encoder_c"]) and net.initialize_hidden_state(5)["encoder_h"].sum() == 0
    assert "encoder.add_layer" not in net.mutation_methods
    with pytest.raises(ValueError):
        ValueNetwork(Box(-1.0, 1.0, (6,))).initialize_hidden_state(1)
    with pytest.raises(NotImplementedError):
        ValueNetwork(Box(-1.0, 1.0, (6,)), recurrent=True, simba=True)

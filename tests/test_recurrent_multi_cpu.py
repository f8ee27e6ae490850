"""StochasticActor over MultiDiscrete and MultiBinary spaces: recurrent PPO's torch path, the GPU tests' reference."""

import numpy as np
import pytest
import torch

from agilerl_amd.envs import Box, MultiBinary, MultiDiscrete
from agilerl_amd.networks.actors import StochasticActor
from agilerl_amd.population.nets import bernoulli_head, multi_categorical

OBS = Box(-np.inf, np.inf, (4,))


@pytest.mark.parametrize("space", [MultiDiscrete([3, 1, 4]), MultiBinary(5)], ids=["multidiscrete", "multibinary"])
def test_actor_head_is_the_population_head(space):
    torch.manual_seed(0)
    actor = StochasticActor(OBS, space, encoder_config={"hidden_state_size": 16}, recurrent=True).double()
    width = int(space.nvec.sum()) if hasattr(space, "nvec") else space.n
    assert actor.output_size == width
    hidden = {k: v.double() for k, v in actor.initialize_hidden_state(batch_size=6).items()}
    latent, _ = actor.extract_features(torch.randn(6, 4, dtype=torch.float64), hidden_state=hidden)
    mask = torch.rand(6, width) > 0.3
    mask[:, 0] = mask[:, 3] = mask[:, 4] = True  # a legal logit in every component
    with torch.no_grad():
        action, log_prob, entropy = actor.forward_head(latent, action_mask=mask)
    logits = actor.head_net.logits
    assert torch.equal(logits[~mask], torch.full_like(logits[~mask], -1e8))
    if hasattr(space, "nvec"):
        assert action.shape == (6, 3) and (action >= 0).all() and (action < torch.as_tensor(space.nvec)).all()
        want = multi_categorical(logits, space.nvec.tolist(), action)
    else:
        assert action.shape == (6, 5) and ((action == 0) | (action == 1)).all() and not action[~mask].any()
        want = bernoulli_head(logits, action)
    assert torch.equal(log_prob, want[0]) and torch.equal(entropy, want[1])
    assert torch.equal(actor.action_log_prob(action.float()), want[0])


def test_other_shapes_still_raise():
    for space in (MultiDiscrete([[2, 2], [3, 3]]), Box(-1.0, 1.0, (2, 2))):
        with pytest.raises(NotImplementedError):
            StochasticActor(OBS, space, recurrent=True)

"""The shared-encoder head kernels (agx_recurrent_heads_forward_shared / _backward_shared, csrc/recurrent_heads.hip)
against float64 autograd of the shared graph on the CPU: one latent feeds both heads, so the two heads' gradients
meet in it.

Error measure and bound as tests/test_lstm_gpu.py: max |a - ref| / max |ref| per tensor, at most 4 x the float32
CPU modules' own error against float64 on the same inputs, + 8 * 2^-23.  The largest ratios seen are in DESIGN 4.17."""

import copy

import pytest
import torch

from agilerl_amd import kernels as K
from agilerl_amd.envs import Box, Discrete, MultiBinary, MultiDiscrete
from tests.test_recurrent_heads_gpu import _check, _names
from tests.test_recurrent_shared_step_gpu import legal_mask, shared_pair

pytestmark = pytest.mark.gpu

# (Bs, L, H, latent, (actor head, its LayerNorm), (critic head, its LayerNorm), space, mask, output activation,
# rows with zero upstream gradients, the critic alone carries the gradient): the issue's table and, last, case 3
# with g_log_prob = g_entropy = 0
CASES = [(1, 1, 16, 8, ([16], False), ([16], False), Discrete(2), False, "ReLU", (), False),
         (3, 11, 48, 24, ([32], True), ([16], False), Discrete(5), True, "ReLU", (), False),
         (3, 11, 64, 32, ([64, 64], False), ([24], True), Box(-1.0, 1.0, (6,)), False, "Tanh", (), False),
         (2, 17, 32, 16, ([16], False), ([16], False), MultiDiscrete([2] * 16), False, "ReLU", (), False),
         (4, 2, 80, 24, ([16], False), ([16], False), MultiBinary(17), True, "Identity", (2, 3, 4), False),
         (3, 11, 64, 32, ([64, 64], False), ([24], True), Box(-1.0, 1.0, (6,)), False, "Tanh", (), True)]


def _reference(actor, critic, h, actions, mask, ups, names, dtype):
    """The shared graph on the CPU in ``dtype`` -> float64 [log_prob, entropy, value], [dh_top, the named gradients]."""
    actor, critic = (copy.deepcopy(n).to("cpu", dtype) for n in (actor, critic))
    x = h.to(dtype).requires_grad_()
    m, name = actor.encoder.model, actor.encoder.name
    latent = m[f"{name}_output_activation"](m[f"{name}_lstm_output"](x))
    _, _, entropy = actor.forward_head(latent, action_mask=mask, sample=False)
    logp = actor.action_log_prob(actions.to(dtype) if actions.dim() == 2 else actions)
    value = critic.head_net(latent).squeeze(-1)
    (logp * ups[0].to(dtype) + entropy * ups[1].to(dtype) + value * ups[2].to(dtype)).sum().backward()
    named = {**dict(actor.named_parameters(prefix="actor")), **dict(critic.named_parameters(prefix="critic"))}
    return [t.detach().double() for t in (logp, entropy, value)], \
        [t.grad.double() for t in (x, *(named[k] for k in names))]


def _launch(actor, critic, h, actions, mask, ups):
    *out, saved = K.recurrent_heads_forward(actor, critic, (h,), actions, mask)
    dh, none, grads = K.recurrent_heads_backward(actor, critic, (h,), actions, mask, saved, *ups)
    assert none is None
    return out, [dh, *grads]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: str(c[:4]) + ("critic" if c[-1] else ""))
def built(request):
    """Per case: the device copies, one forward and backward launch, and both references (never modified)."""
    Bs, L, H, latent, ahead, chead, space, masked, out_act, zero, critic_only = request.param
    actor, critic, twin = shared_pair(4, H, 1, latent, ahead, chead, space, out_act, 1000 * Bs + H)
    R = Bs * L
    h = 0.5 * torch.randn(R, H)
    if isinstance(space, Box):
        actions = torch.randn(R, space.shape[0])
    elif isinstance(space, Discrete):
        actions = torch.randint(0, space.n, (R,)).float()
    else:
        actions = torch.randint(0, 2, (R, 16 if isinstance(space, MultiDiscrete) else space.n)).float()
    mask = legal_mask(space, R) if masked else None
    if masked and isinstance(space, Discrete):
        mask[torch.arange(R), actions.long()] = True
    ups = [torch.randn(R) * (0.0 if critic_only and i < 2 else 1.0) for i in range(3)]
    for u in ups:
        u[list(zero)] = 0
    host = (h, actions, mask, ups)
    nets = [n.to("cuda") for n in (actor, critic, twin)]
    dev = (nets[0], nets[1], h.cuda(), actions.cuda(), None if mask is None else mask.cuda(), [u.cuda() for u in ups])
    names = _names(*nets[:2])
    assert not any("critic.encoder" in n for n in names)  # one output Linear, the actor's
    ref, base = (_reference(actor, critic, *host, names, d) for d in (torch.float64, torch.float32))
    return request.param, dev, nets[2], names, _launch(*dev), base, ref


def test_parity(built):
    case, _, _, names, got, base, ref = built
    _check(case, ["log_prob", "entropy", "value"], got[0], base[0], ref[0])
    _check(case, ["dh_top", *names], got[1], base[1], ref[1])
    assert not got[1][0][list(case[-2])].any()  # rows without an upstream gradient add nothing
    if case[-1]:  # the value path alone reaches the encoder
        assert got[1][0].any() and got[1][1 + names.index("actor.encoder.model.shared_encoder_lstm_output.weight")].any()


def test_forward_bits_and_repeat(built):
    _, (actor, critic, h, actions, mask, ups), twin, _, got, _, _ = built
    want = K.recurrent_heads_forward(actor, twin, (h, h), actions, mask, save=False)[:3]
    assert all(torch.equal(u, v) for u, v in zip(got[0], want))
    again = _launch(actor, critic, h, actions, mask, ups)
    assert all(torch.equal(u, v) for u, v in zip(got[0] + got[1], again[0] + again[1]))

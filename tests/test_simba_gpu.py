"""The fused SimBa encoder (csrc/simba.hip through modules/simba.py) against the
same torch modules in float64, its determinism, its fallbacks, and DQN / DDPG /
TD3 agents built on it."""

import copy

import numpy as np
import pytest
import torch

from agilerl_amd.modules.simba import EvolvableSimBa, simba_encoder

pytestmark = pytest.mark.gpu

# (in, H, scale, blocks, out, B), output activation
CASES = [((6, 16, 4, 1, 8, 5), "ReLU"), ((11, 40, 4, 2, 20, 33), "ReLU"), ((8, 128, 4, 2, 32, 64), "ReLU"),
         ((9, 48, 2, 3, 16, 17), "ReLU"), ((17, 496, 4, 1, 128, 64), "ReLU"), ((8, 32, 4, 1, 8, 1024), "ReLU"),
         ((11, 40, 4, 2, 20, 33), None)]
GATE_MARGIN = 2e-4


def _build(case, act, seed, device):
    """The encoder (LayerNorm affines away from identity), rows whose ReLU
    gates all sit clear of zero in float64, and the loss weights g."""
    nin, H, scale, blocks, nout, B = case
    torch.manual_seed(seed)
    net = EvolvableSimBa(nin, nout, H, blocks, output_activation=act, scale_factor=scale, max_blocks=4)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if "norm" in k:
                p.copy_((1.0 if k.endswith("weight") else 0.0) + 0.3 * torch.randn(p.shape, generator=gen))
    ref = copy.deepcopy(net).double()
    gates = []
    hooks = [m.register_forward_hook(lambda _m, _i, o: gates.append(o.abs().min(dim=1).values))
             for k, m in ref.model.named_modules() if k.endswith("linear1") or (act and k.endswith("layer_output"))]
    cand = torch.randn(2 * B, nin, generator=gen)
    with torch.no_grad():
        ref.model(cand.double())
    for h in hooks:
        h.remove()
    keep = torch.stack(gates).min(dim=0).values > GATE_MARGIN
    assert int(keep.sum()) >= B, f"{case}: {int(keep.sum())} of {2 * B} candidate rows clear of the ReLU gates"
    x = cand[keep][:B].contiguous()
    g = torch.randn(B, nout, generator=gen)
    return net.to(device), ref, x, g


def _run(net, x, g, fused=True):
    x = x.clone().requires_grad_(True)
    net.zero_grad(set_to_none=True)
    y = simba_encoder(net, x) if fused else net.model(x)
    assert y is not None
    (y * g).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in net.parameters()]


@pytest.mark.parametrize("case,act", CASES)
def test_fused_encoder_matches_float64(case, act):
    net, ref, x, g = _build(case, act, seed=sum(case), device="cuda")
    got = _run(net, x.cuda(), g.cuda())
    want = _run(ref, x.double(), g.double(), fused=False)
    names = ["y", "dx"] + [k for k, _ in net.named_parameters()]
    for i, (name, a, b) in enumerate(zip(names, got, want)):
        err = float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))
        print(f"{case} {name}: {err:.3e}")
        assert err <= (2e-5 if i == 0 else 5e-5), (case, name, err)


def test_two_runs_are_bit_identical():
    net, _, x, g = _build(CASES[2][0], "ReLU", seed=3, device="cuda")
    a, b = _run(net, x.cuda(), g.cuda()), _run(net, x.cuda(), g.cuda())
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_fallbacks(monkeypatch):
    net, _, x, _ = _build(CASES[0][0], "ReLU", seed=4, device="cuda")
    x = x.cuda()
    assert simba_encoder(net, x) is not None
    assert simba_encoder(net, torch.zeros(1025, 6, device="cuda")) is None
    assert simba_encoder(net, torch.zeros(1024, 6, device="cuda")) is not None
    assert simba_encoder(net, x.double()) is None
    tanh = EvolvableSimBa(6, 8, 16, 1, output_activation="Tanh", device="cuda")
    assert simba_encoder(tanh, x) is None and tanh(x).shape == (5, 8)
    assert simba_encoder(EvolvableSimBa(6, 8, 16, 1, output_activation="ReLU", device="cuda"), x) is not None
    h = net.model[0].register_forward_hook(lambda *a: None)
    assert simba_encoder(net, x) is None
    h.remove()
    assert simba_encoder(net, x) is not None
    monkeypatch.setenv("AGX_SIMBA", "0")
    assert simba_encoder(net, x) is None
    monkeypatch.delenv("AGX_SIMBA")
    assert simba_encoder(net, x) is not None


def test_dqn_learns_the_same_with_and_without_the_fused_encoder(monkeypatch):
    from agilerl_amd.algorithms import DDPG, DQN, TD3
    from agilerl_amd.algorithms.flat_state import flat_state
    from agilerl_amd.envs import Box, Discrete

    cfg = {"simba": True, "encoder_config": {"hidden_size": 64, "num_blocks": 1}}
    torch.manual_seed(7)
    a = DQN(Box(-np.inf, np.inf, (8,)), Discrete(4), batch_size=64, lr=1e-3, net_config=cfg)
    r = copy.deepcopy(a)
    from agilerl_amd.modules import simba

    taken = []  # the fused path inside learn (eager call; the replays run its captured launches)
    real = simba.simba_encoder
    monkeypatch.setattr(simba, "simba_encoder", lambda m, x: taken.append(real(m, x)) or taken[-1])
    rng = np.random.default_rng(3)
    for _ in range(3):  # eager, then captured and replayed
        e = {"obs": rng.standard_normal((64, 8)).astype(np.float32), "action": rng.integers(0, 4, (64, 1)),
             "reward": rng.standard_normal((64, 1)).astype(np.float32),
             "next_obs": rng.standard_normal((64, 8)).astype(np.float32),
             "done": (rng.random((64, 1)) < 0.2).astype(np.float32)}
        a.learn(e)
        with monkeypatch.context() as mp:
            mp.setenv("AGX_SIMBA", "0")
            r.learn(e)
    assert flat_state(a) is not None
    assert any(t is not None for t in taken) and any(t is None for t in taken)  # the agent fused, the twin fell back
    for net, twin in ((a.actor, r.actor), (a.actor_target, r.actor_target)):
        for (k, p), q in zip(net.state_dict().items(), twin.state_dict().values()):
            assert float((p - q).abs().max()) <= 1e-4 * float(q.abs().max()), k
    for cls in (TD3, DDPG):
        agent = cls(Box(-np.inf, np.inf, (8,)), Box(-1.0, 1.0, (2,)), net_config={"simba": True})
        assert np.asarray(agent.get_action(np.zeros((1, 8), np.float32))).shape[-1] == 2

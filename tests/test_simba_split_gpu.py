"""The split SimBa kernels (plans (S, R, Q) of include/agx_simba.h) against the
same modules in float64, and what the ticket reduction promises: plan (1, 1, 1)
is the whole kernels, runs repeat bit for bit, and captured replays do too."""

import pytest
import torch

from agilerl_amd.modules.simba import simba_encoder
from tests.test_simba_gpu import _build

pytestmark = pytest.mark.gpu

# (in, H, scale, blocks, out, B), output activation, plan (S, R, Q)
CASES = [((6, 16, 4, 1, 8, 5), "ReLU", (3, 1, 1)), ((11, 40, 4, 2, 20, 33), None, (2, 2, 2)),
         ((9, 50, 2, 3, 16, 17), "ReLU", (5, 1, 2)), ((8, 128, 4, 2, 32, 64), "ReLU", (4, 4, 1)),
         ((17, 496, 4, 1, 128, 64), "ReLU", (16, 2, 2)), ((8, 32, 4, 1, 8, 1024), "ReLU", (1, 4, 4)),
         ((4, 512, 4, 1, 4, 16), "ReLU", (16, 1, 1))]


def _run(net, x, g, plan="torch"):
    x = x.clone().requires_grad_(True)
    net.zero_grad(set_to_none=True)
    y = net.model(x) if plan == "torch" else simba_encoder(net, x, plan=plan)
    assert y is not None
    (y * g).sum().backward()
    return [y.detach(), x.grad] + [p.grad for p in net.parameters()]


def _case2():
    case, act, plan = CASES[1]
    net, _, x, g = _build(case, act, seed=sum(case), device="cuda")
    return net, x.cuda(), g.cuda(), plan


@pytest.mark.parametrize("case,act,plan", CASES)
def test_split_encoder_matches_float64(case, act, plan):
    net, ref, x, g = _build(case, act, seed=sum(case), device="cuda")
    got = _run(net, x.cuda(), g.cuda(), plan)
    want = _run(ref, x.double(), g.double())
    names = ["y", "dx"] + [k for k, _ in net.named_parameters()]
    for i, (name, a, b) in enumerate(zip(names, got, want)):
        err = float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))
        print(f"{case} {plan} {name}: {err:.3e}")
        assert err <= (2e-5 if i == 0 else 5e-5), (case, plan, name, err)


def test_whole_plan_through_split_entry_points_has_the_whole_kernels_bits(monkeypatch):
    net, x, g, _ = _case2()
    a = _run(net, x, g, (1, 1, 1))
    monkeypatch.setenv("AGX_SIMBA_SPLIT", "0")
    b = _run(net, x, g, None)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_two_split_runs_are_bit_identical():
    net, x, g, plan = _case2()
    a, b = _run(net, x, g, plan), _run(net, x, g, plan)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_captured_replays_give_the_eager_bits():
    """Three replays of one capture: the ticket counters are back at zero after every launch."""
    net, x, g, plan = _case2()
    want = _run(net, x, g, plan)
    params = list(net.parameters())
    xs = x.clone().requires_grad_(True)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):  # after an eager run, as algorithms/learn_graph.py captures
        y = simba_encoder(net, xs, plan=plan)
        grads = torch.autograd.grad((y * g).sum(), [xs] + params)
    for _ in range(3):
        for t in (y, *grads):
            t.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip([y.detach(), *grads], want))

"""NeuralUCB / NeuralTS on the GPU: agx_bandit_select against the reference's
own get_action steps (tests/golden/bandit_*.npz) and the float64 twin
(tests/bandit_twin.py) at the shapes where its two forms can go wrong, its
argmax rules and Thompson noise, the agents' get_action — eager, captured and
replayed, across updates and a mutation — and learn against a plain-torch
twin, and train_bandits.

The bound on every float32 result is 4 x max(err_ref, 1 float32 ulp of the
value), err_ref being the one-step error of the reference's float32
evaluation against float64 on the same inputs (META_bandit.json for the
golden cases, tests.bandit_twin.ref32 — torch CPU float32 ops — for the
others).  Every comparison is one step deep: the device steps its own matrix
through all T steps and the twin is evaluated on the matrix the device held
before each step; against the reference's recorded float32 outputs the step
starts from the matrix the reference held (two float32 runs drift apart by
their accumulated rounding, which a one-step error does not bound).  Actions
are compared exactly over the whole run: every step keeps the best two legal
scores 64 x err_ref apart, asserted before the device result is looked at.

Two tolerances here are not that bound, on purpose.  The agent-level runs
(_drive) compare the agent's matrix with a twin agent's whose network is
trained by torch's Adam on its own copy: the two networks differ by the
update test's tolerance, so the matrices are held to that tolerance (rtol
1e-4, atol 2e-5, test_cqn_gpu.py's), not to the one-step bound; the kernel's
one-step bound is what the kernel tests above check.  The Thompson score is
held to 4 ulp of the product gamma sqrt(quad) z plus half an ulp of the score:
the half ulp is the score's own final rounding, which is not an error of the
product and exceeds 4 ulp of it whenever |mu| is much larger than the width."""

import glob
import json
import os

import numpy as np
import pytest
import torch

from tests import bandit_twin as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "META_bandit.json")))
CASES = sorted(META["errors"])
RESIDENT = 112  # AGX_BANDIT_RESIDENT_MAX_D (test_bandit_cpu.py checks the header against kernels.py)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _within(tag, got, want, err_ref, extra=0.0):
    d = np.abs(np.asarray(got, np.float64) - want)
    b = T.bound(err_ref, want) + extra
    print(f"{tag}: max err {d.max():.3e}, err_ref {err_ref:.3e}, worst err/bound {np.max(d / b):.3f}")
    assert (d <= b).all(), tag


def _step(h, mu, S_dev, mask, gamma=1.0, bias_one=True, scale=1.0):
    """The twin on the device's matrix as it is, then the kernel -> (twin, action, scores, quad)."""
    from agilerl_amd import kernels as K

    twin = T.select(T.gradients(h, bias_one, scale), mu, S_dev.cpu().numpy(), mask, gamma)
    a, sc, q = K.bandit_select(_dev(h), _dev(mu), S_dev, None if mask is None else _dev(mask), bias_one=bias_one,
                               scale=scale, gamma=gamma)
    return twin, int(a.item()), sc.cpu().numpy(), q.cpu().numpy()


# ---- agx_bandit_select against the reference -------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_kernel_matches_reference_golden(golden, case):
    g, err = golden(case), META["errors"][case]
    D, gamma, masked = g["h"].shape[2] + 1, float(g["gamma"]), bool(g["masked"])
    S = (float(g["lamb"]) * torch.eye(D)).cuda()
    for t in range(len(g["action"])):
        mask = g["mask"][t] if masked else None
        if err["gap"][t] is not None:
            assert err["gap"][t] >= 64 * err["err_ref_scores"][t]
        twin, action, scores, quad = _step(g["h"][t], g["mu"][t], S, mask, gamma)
        assert twin["action"] == int(g["action"][t]) and action == int(g["action"][t]), (case, t)
        _within(f"{case}[{t}] scores", scores, twin["scores"], err["err_ref_scores"][t])
        _within(f"{case}[{t}] quad", quad, twin["quad"], err["err_ref_quad"][t])
        _within(f"{case}[{t}] sigma_inv", S.cpu().numpy(), twin["sigma_inv"], err["err_ref_sigma"][t])
    # the reference's float32 outputs lie within the same distance plus err_ref, step by step from the
    # matrix the reference held
    pre = (float(g["lamb"]) * np.eye(D)).astype(np.float32)
    for t in range(len(g["action"])):
        S = _dev(pre)
        twin, action, scores, _ = _step(g["h"][t], g["mu"][t], S, g["mask"][t] if masked else None, gamma)
        assert action == int(g["action"][t])
        _within(f"{case}[{t}] scores vs reference", scores, g["action_values"][t].astype(np.float64),
                err["err_ref_scores"][t], extra=err["err_ref_scores"][t])
        _within(f"{case}[{t}] sigma_inv vs reference", S.cpu().numpy(), g["sigma_inv"][t].astype(np.float64),
                err["err_ref_sigma"][t], extra=err["err_ref_sigma"][t])
        pre = g["sigma_inv"][t]


def _run_inputs(tag, steps, bias_one=True, strided=False):
    from agilerl_amd import kernels as K

    D = steps[0]["h"].shape[1] + int(bias_one)
    S = torch.eye(D).cuda()
    for t, st in enumerate(steps):
        assert st["twin"]["gap"] >= 64 * st["err_scores"]  # the drawn inputs
        pre = S.cpu().numpy()
        twin = T.select(T.gradients(st["h"], bias_one), st["mu"], pre, st["mask"])
        assert twin["gap"] >= 64 * st["err_scores"] and twin["action"] == st["twin"]["action"]  # and on this matrix
        h = _dev(st["h"])
        if strided:  # rows 5 floats apart from dense, a sentinel between them
            buf = torch.full((h.shape[0], h.shape[1] + 5), float("nan"), device="cuda")
            buf[:, :h.shape[1]] = h
            h = buf[:, :h.shape[1]]
            assert not h.is_contiguous()
        a, sc, q = K.bandit_select(h, _dev(st["mu"]), S, None if st["mask"] is None else _dev(st["mask"]),
                                   bias_one=bias_one)
        assert int(a.item()) == twin["action"], (tag, t)
        _within(f"{tag}[{t}] scores", sc.cpu().numpy(), twin["scores"], st["err_scores"])
        _within(f"{tag}[{t}] quad", q.cpu().numpy(), twin["quad"], st["err_quad"])
        _within(f"{tag}[{t}] sigma_inv", S.cpu().numpy(), twin["sigma_inv"], st["err_sigma"])


@pytest.mark.parametrize("A,D,steps", [(33, RESIDENT, 8), (1, RESIDENT, 8), (33, RESIDENT + 1, 8),
                                       (1, RESIDENT + 1, 8), (7, 501, 4), (2, 1025, 1)])
def test_kernel_matches_twin_at_form_boundaries(A, D, steps):
    """The last resident D and the first streaming D (a part-filled arm tile
    and a single arm), D = 501 (two column tiles, the second part-filled), and
    the cap."""
    _run_inputs(f"A={A} D={D}", T.inputs(A, D - 1, steps, seed=100 + D, masked=A > 1))


@pytest.mark.parametrize("D", [33, RESIDENT + 1])
def test_kernel_explicit_gradient_matrix(D):
    _run_inputs(f"explicit g D={D}", T.inputs(9, D, 4, seed=7 + D, bias_one=False), bias_one=False)


@pytest.mark.parametrize("D", [33, RESIDENT + 1])
def test_kernel_strided_h(D):
    _run_inputs(f"strided D={D}", T.inputs(9, D - 1, 3, seed=11 + D, masked=True), strided=True)


def test_scale_multiplies_the_gradient():
    st = T.inputs(5, 32, 1, seed=3)[0]
    S = (2.0 * torch.eye(33)).cuda()
    twin, action, scores, quad = _step(st["h"], st["mu"], S, None, gamma=0.7, scale=0.5)
    assert action == twin["action"]
    _within("scale quad", quad, twin["quad"], 0.0)
    _within("scale scores", scores, twin["scores"], 0.0)
    _within("scale sigma_inv", S.cpu().numpy(), twin["sigma_inv"], 0.0)


@pytest.mark.parametrize("A,D", [(10, 33), (20, 200)])
def test_two_runs_give_the_same_bits(A, D):
    from agilerl_amd import kernels as K

    st = T.inputs(A, D - 1, 1, seed=5)[0]
    h, mu = _dev(st["h"]), _dev(st["mu"])
    S1 = (torch.eye(D) + 0.01 * torch.randn(D, D, generator=torch.Generator().manual_seed(0))).cuda()
    S2 = S1.clone()
    # an asymmetric matrix: u = S v and w = S^T v differ, so a swapped or shared product shows
    twin = T.select(T.gradients(st["h"]), st["mu"], S1.cpu().numpy())
    out1, out2 = K.bandit_select(h, mu, S1), K.bandit_select(h, mu, S2)
    assert all(torch.equal(x, y) for x, y in zip(out1, out2)) and torch.equal(S1, S2)
    _within(f"asymmetric D={D} quad", out1[2].cpu().numpy(), twin["quad"], 0.0)
    _within(f"asymmetric D={D} sigma_inv", S1.cpu().numpy(), twin["sigma_inv"], 0.0)
    out3 = K.bandit_select(h, mu, S1)  # a second step on the updated matrix differs
    assert not torch.equal(out3[2], out1[2])


def test_above_the_cap_the_entry_point_refuses_and_torch_takes_over():
    from agilerl_amd import _lib
    from agilerl_amd import kernels as K

    lib = _lib.load()
    for A, H in ((2, 1025), (1025, 4)):
        D = H + 1
        h, mu, S = torch.zeros(A, H, device="cuda"), torch.zeros(A, device="cuda"), torch.eye(D, device="cuda")
        out = torch.zeros(2 * A + 2, device="cuda")
        act, ws = torch.full((1,), -7, dtype=torch.int64, device="cuda"), torch.zeros(64, device="cuda")
        assert lib.agx_bandit_workspace_bytes(A, D) == 0
        rc = lib.agx_bandit_select(h.data_ptr(), H, mu.data_ptr(), S.data_ptr(), None, A, H, 1, 1.0, 1.0, 0, 0, None,
                                   out.data_ptr(), out[A:].data_ptr(), act.data_ptr(), ws.data_ptr(), _lib.stream())
        assert rc == -1 and (b"exceeds" in lib.agx_last_error() or b"<= A <=" in lib.agx_last_error())
        torch.cuda.synchronize()
        assert int(act) == -7 and torch.equal(S, torch.eye(D, device="cuda"))  # nothing launched
    st = T.inputs(2, 1025, 1, seed=2)[0]  # D = 1026
    S = torch.eye(1026).cuda()
    twin, action, scores, quad = _step(st["h"], st["mu"], S, None)
    assert action == twin["action"]
    _within("fallback scores", scores, twin["scores"], st["err_scores"])
    _within("fallback quad", quad, twin["quad"], st["err_quad"])
    _within("fallback sigma_inv", S.cpu().numpy(), twin["sigma_inv"], st["err_sigma"])


@pytest.mark.parametrize("D", [33, RESIDENT + 1])
def test_nan_ties_and_masks_follow_numpy(D):
    from agilerl_amd import kernels as K

    A, H = 130, D - 1
    rng = np.random.default_rng(D)
    h = np.abs(rng.standard_normal((A, H))).astype(np.float32)
    mu = rng.standard_normal(A).astype(np.float32) - 50.0

    def run(h, mu, mask=None):
        S = torch.eye(D).cuda()
        a, sc, _ = K.bandit_select(_dev(h), _dev(mu), S, None if mask is None else _dev(mask))
        want = T.argmax(sc.cpu().numpy().astype(np.float64), mask)  # numpy's own rule on the device's scores
        return int(a.item()), want, S

    # two equal top scores: the lower index, within a lane's two passes (5, 69) and across lanes (70, 3)
    for pair in ((5, 69), (70, 3), (128, 129)):
        h2, mu2 = h.copy(), mu.copy()
        h2[pair[1]] = h2[pair[0]]
        mu2[list(pair)] = 100.0
        a, want, _ = run(h2, mu2)
        assert a == want == min(pair)
        mask = np.ones(A, np.uint8)
        mask[min(pair)] = 0  # the lower one masked: the other
        a, want, _ = run(h2, mu2, mask)
        assert a == want == max(pair)
    # a NaN in mu selects that arm, the first of two, unless it is masked
    mu2 = mu.copy()
    mu2[[77, 9]] = np.nan
    a, want, S = run(h, mu2)
    assert a == want == 9
    assert torch.isfinite(S).all()  # the update used arm 9's finite gradient
    mask = np.ones(A, np.uint8)
    mask[9] = 0
    assert run(h, mu2, mask)[0] == 77
    mask[77] = 0
    a, want, _ = run(h, mu2, mask)
    assert a == want and a not in (9, 77)
    # every arm masked: 0, as np.ma gives; a mask byte other than 1 is not legal
    a, want, _ = run(h, mu, np.zeros(A, np.uint8))
    assert a == want == 0
    mask = np.full(A, 2, np.uint8)
    mask[40] = 1
    assert run(h, mu, mask)[0] == 40


# ---- Thompson sampling ---------------------------------------------------------------------------------
def test_thompson_scores_counter_and_moments():
    from agilerl_amd import kernels as K

    A, D, gamma, seed = 64, 33, 0.8, 0x5EED5EED1234
    steps = T.inputs(A, D - 1, 1, seed=21)
    h, mu = _dev(steps[0]["h"]), _dev(steps[0]["mu"])
    # the twin's own draws meet the moment test first
    z_twin = np.stack([T.normals(A, seed, (3 << 32) + c) for c in range(64)])
    assert abs(z_twin.mean()) < 5 / np.sqrt(z_twin.size) and 0.85 <= z_twin.var() <= 1.15
    counter = torch.tensor([3 << 32], dtype=torch.int64, device="cuda")  # the high word is live
    S = torch.eye(D).cuda()
    zs = []
    for c in range(64):
        pre = S.cpu().numpy()
        twin = T.select(T.gradients(steps[0]["h"]), steps[0]["mu"], pre, None, gamma, z=z_twin[c])
        a, sc, q = K.bandit_select(h, mu, S, thompson=True, seed=seed, counter=counter, gamma=gamma)
        assert int(counter) == (3 << 32) + c + 1  # one per call
        product = gamma * np.sqrt(twin["quad"]) * z_twin[c]
        d = np.abs(sc.cpu().numpy().astype(np.float64) - twin["scores"])
        # 4 ulp of the product (the device's float32 log / sqrt / cospi) and the score's own final rounding
        assert (d <= 4 * T.ulp(product) + 0.5 * T.ulp(twin["scores"])).all(), (c, (d / T.ulp(product)).max())
        _within(f"thompson[{c}] quad", q.cpu().numpy(), twin["quad"], 0.0)
        gap = np.sort(twin["scores"])[::-1]
        if gap[0] - gap[1] > 64 * 4 * T.ulp(product).max():
            assert int(a) == twin["action"]
        zs.append((sc.cpu().numpy().astype(np.float64) - steps[0]["mu"]) / (gamma * np.sqrt(q.cpu().numpy())))
        if c >= 8:  # the rest from a fresh matrix: the moments need the draws, not the run
            S = torch.eye(D).cuda()
    zs = np.stack(zs)
    print(f"thompson: mean {zs.mean():.4f}, var {zs.var():.4f} over {zs.size} draws")
    assert abs(zs.mean()) < 5 / np.sqrt(4096) and 0.85 <= zs.var() <= 1.15
    # another seed, other noise; the same seed and counter, the same bits
    c1 = torch.tensor([5], dtype=torch.int64, device="cuda")
    c2, c3 = c1.clone(), c1.clone()
    S = torch.eye(D).cuda()
    s1 = K.bandit_select(h, mu, S.clone(), thompson=True, seed=1, counter=c1)[1]
    s2 = K.bandit_select(h, mu, S.clone(), thompson=True, seed=2, counter=c2)[1]
    s3 = K.bandit_select(h, mu, S.clone(), thompson=True, seed=1, counter=c3)[1]
    assert torch.equal(s1, s3) and (s1 != s2).float().mean() > 0.9
    with pytest.raises(TypeError):
        K.bandit_select(h, mu, S, thompson=True, seed=1)  # Thompson needs the counter


def test_two_thompson_agents_draw_different_noise():
    """Through the agents' own seeds: equal networks, matrices and context,
    different indices -> different scores; the same index -> the same bits.
    A UCB agent's call leaves its counter alone, on either route."""
    from agilerl_amd.algorithms import NeuralTS, NeuralUCB

    env = _env()
    torch.manual_seed(3)
    a = NeuralTS(env.observation_space, env.action_space, device="cuda")
    b, c = a.clone(a.index + 1), a.clone()
    assert a.noise_seed != b.noise_seed and a.noise_seed == c.noise_seed
    ctx = env.reset()
    for agent in (a, b, c):
        agent.get_action(ctx)
        assert int(agent.ts_counter) == 1
    assert torch.equal(a.last_quad, b.last_quad) and torch.equal(a.last_scores, c.last_scores)
    assert (a.last_scores != b.last_scores).all()
    torch.manual_seed(3)
    u = NeuralUCB(env.observation_space, env.action_space, device="cuda")
    u.get_action(ctx)
    u.get_action(ctx)
    assert int(u.ts_counter) == 0


def test_binding_checks_shapes_and_devices():
    from agilerl_amd import kernels as K

    h, mu, S = torch.zeros(4, 8, device="cuda"), torch.zeros(4, device="cuda"), torch.eye(9, device="cuda")
    with pytest.raises(ValueError):
        K.bandit_select(h, mu, S[:8, :8].contiguous())
    with pytest.raises(ValueError):
        K.bandit_select(h, mu[:3], S)
    with pytest.raises(ValueError):
        K.bandit_select(h.cpu(), mu, S)
    with pytest.raises(TypeError):
        K.bandit_select(h.double(), mu, S)
    with pytest.raises(ValueError):
        K.bandit_select(h[:, :1].expand(4, 8), mu, S)  # overlapping rows
    with pytest.raises(TypeError):
        K.bandit_select(h, mu, S, torch.ones(4, device="cuda"))  # a float mask


# ---- the agents ---------------------------------------------------------------------------------------------
def _env(seed=3):
    from agilerl_amd.envs import SyntheticBanditEnv

    return SyntheticBanditEnv(arms=4, features=6, seed=seed)


def _graphs(agent):
    from agilerl_amd.algorithms import neural_ucb_bandit as N

    slot = N._ACT_GRAPHS.get(agent)
    return [] if slot is None else [k for k, e in slot["table"].items() if e.graph is not None]


def _learn_graphs(agent):
    from agilerl_amd.algorithms import learn_graph
    from agilerl_amd.algorithms.flat_state import flat_state

    table = learn_graph._GRAPHS.get(flat_state(agent), {})
    return [k for k, ent in table.items() if k[0] == "bandit" and ent.graph is not None]


def _batch(gen, B=16):
    return {"obs": torch.randn(B, 24, generator=gen).cuda(), "reward": (torch.rand(B, 1, generator=gen) < 0.3).float().cuda()}


def _drive(agent, twin, env, steps, gen, mask_every=0):
    """``steps`` env steps of agent and twin side by side, a learn after every
    fourth -> the number of calls that came out of a captured graph.  Asserts equal actions, the gap
    condition on the twin, and matrices within the update test's tolerance."""
    ctx = env.reset()
    replays = 0
    for t in range(steps):
        mask = None
        if mask_every and t % mask_every == 1:
            mask = np.ones(4, np.int64)
            mask[t % 4] = 0
        want, gap, err = twin.act(ctx, mask)
        assert gap >= 64 * err, (t, gap, err)
        action = agent.get_action(ctx, action_mask=mask)
        # the call came out of a graph iff one exists for its key now (captured in this call, or before)
        replays += int(any(k[0] == (4, 24) and k[2] == (mask is not None) for k in _graphs(agent)))
        assert isinstance(action, int) and action == want, t
        torch.testing.assert_close(agent.sigma_inv, twin.agent.sigma_inv, rtol=1e-4, atol=2e-5)
        ctx, _ = env.step(action)
        if t % 4 == 3:
            experiences = _batch(gen)
            loss, twin_loss = agent.learn(experiences), twin.learn(experiences)
            assert np.isfinite(loss) and abs(loss - twin_loss) <= 1e-4 * abs(twin_loss) + 2e-5
    return replays


def _agent_and_twin(seed):
    from agilerl_amd.algorithms import NeuralUCB

    env = _env()
    torch.manual_seed(seed)
    agent = NeuralUCB(env.observation_space, env.action_space, device="cuda", lr=1e-3, batch_size=16)
    return env, agent, T.Twin.of(agent)


def _first_seed_with_gaps(steps=32):
    """The twin alone, seed by seed, until every step's gap clears 64 x the
    float32 error: the inputs of the agent tests, fixed before any device
    result is looked at."""
    for seed in range(20):
        env, agent, twin = _agent_and_twin(seed)
        gen = torch.Generator().manual_seed(seed)
        ctx, ok = env.reset(), True
        for t in range(steps):
            mask = None
            if t % 5 == 1:
                mask = np.ones(4, np.int64)
                mask[t % 4] = 0
            action, gap, err = twin.act(ctx, mask)
            if not gap >= 64 * err:
                ok = False
                break
            ctx, _ = env.step(action)
            if t % 4 == 3:
                twin.learn(_batch(gen))
        if ok:
            return seed
    raise AssertionError("no seed keeps every gap above 64 x the float32 error")


@pytest.fixture(scope="module")
def agent_seed():
    return _first_seed_with_gaps()


@pytest.mark.parametrize("graphs", [True, False])
def test_get_action_matches_twin_eager_and_replayed(graphs, agent_seed, monkeypatch):
    if not graphs:
        monkeypatch.setenv("AGX_LEARN_GRAPH", "0")
    env, agent, twin = _agent_and_twin(agent_seed)
    replays = _drive(agent, twin, env, 32, torch.Generator().manual_seed(agent_seed), mask_every=5)
    if graphs:
        # the flat state re-points the parameters at the first learn: the graphs of before are dropped,
        # later ones survive the updates (the weights change under them)
        assert replays >= 16 and len(_graphs(agent)) >= 1 and len(_learn_graphs(agent)) == 1
    else:
        assert replays == 0 and _graphs(agent) == [] and _learn_graphs(agent) == []
    for p1, p2 in zip(agent.actor.parameters(), twin.actor.parameters()):
        torch.testing.assert_close(p1, p2, rtol=1e-4, atol=2e-5)


def test_get_action_after_a_mutation_that_changes_H(agent_seed):
    from agilerl_amd.algorithms import neural_ucb_bandit as N

    env, agent, twin = _agent_and_twin(agent_seed)
    gen = torch.Generator().manual_seed(agent_seed)
    _drive(agent, twin, env, 8, gen)
    assert len(_graphs(agent)) == 1
    stale = N._ACT_GRAPHS[agent]["sig"]
    old = agent._exp_sizes()
    assert agent.actor.apply_mutation_dict("head_net.add_node", {"hidden_layer": 0, "numb_new_nodes": 16})[0] == \
        "head_net.add_node"
    agent._reinit_bandit_grads(old)
    agent.mutation_hook()
    agent.reinit_optimizers()
    twin = T.Twin.of(agent)  # copies of the mutated network (its new weights are drawn at random) and matrix
    assert agent.numel == 49 and agent.sigma_inv.shape == (49, 49) and agent._graph_signature() != stale
    replays = _drive(agent, twin, env, 12, gen)
    assert N._ACT_GRAPHS[agent]["sig"] != stale and replays >= 4  # the stale graph went, new ones replay
    assert all(k[0] == (4, 24) for k in _graphs(agent))


def test_autograd_route_on_the_gpu():
    from agilerl_amd.algorithms import NeuralUCB
    from agilerl_amd.networks.base import mlp_net_config

    env = _env()
    torch.manual_seed(1)
    agent = NeuralUCB(env.observation_space, env.action_space, device="cuda",
                      net_config={"head_config": mlp_net_config([32], output_activation="Tanh")})
    assert not agent.closed_form()
    ctx = env.reset()
    for _ in range(3):
        mu, g = agent.arm_gradients(agent._obs(ctx))
        twin = T.select(g.cpu().numpy().astype(np.float64), mu.cpu().numpy(), agent.sigma_inv.cpu().numpy(), None, 1.0)
        action = agent.get_action(ctx)
        if twin["gap"] > 1e-4:
            assert action == twin["action"]
        _within("autograd route sigma_inv", agent.sigma_inv.cpu().numpy(), twin["sigma_inv"], 0.0)
        ctx, _ = env.step(action)
    assert _graphs(agent) == []


@pytest.mark.parametrize("name", ["NeuralUCB", "NeuralTS"])
def test_learn_matches_twin(name, monkeypatch):
    from agilerl_amd import algorithms

    env = _env()
    torch.manual_seed(0)
    agent = getattr(algorithms, name)(env.observation_space, env.action_space, device="cuda", lr=1e-3, batch_size=16)
    eager = agent.clone()
    twin = T.Twin.of(agent)
    gen = torch.Generator().manual_seed(1)
    batches = [_batch(gen) for _ in range(8)]
    for k, experiences in enumerate(batches):
        loss, twin_loss = agent.learn(experiences), twin.learn(experiences)
        print(f"update {k}: loss {loss:.7f}, twin {twin_loss:.7f}")
        assert np.isfinite(loss) and abs(loss - twin_loss) <= 1e-4 * abs(twin_loss) + 2e-5
        assert len(_learn_graphs(agent)) == (0 if k == 0 else 1)  # eager, captured, then replayed
    for p1, p2 in zip(agent.actor.parameters(), twin.actor.parameters()):
        torch.testing.assert_close(p1, p2, rtol=1e-4, atol=2e-5)
    assert not torch.equal(agent.theta_0, torch.cat([p.detach().flatten() for p in agent.exp_layer.parameters()]))
    steps = {float(s["step"]) for s in agent.optimizer.state_dict()["state"].values()}
    assert steps == {8.0}
    monkeypatch.setenv("AGX_LEARN_GRAPH", "0")
    for experiences in batches:
        eager.learn((experiences["obs"], experiences["reward"]))  # the (obs, reward) pair
    assert _learn_graphs(eager) == []
    for p1, p2 in zip(agent.actor.parameters(), eager.actor.parameters()):
        torch.testing.assert_close(p1, p2, rtol=1e-4, atol=2e-5)


def test_train_bandits_gpu(tmp_path):
    from agilerl_amd.algorithms import NeuralTS
    from agilerl_amd.components import ReplayBuffer
    from agilerl_amd.hpo.mutation import Mutations
    from agilerl_amd.hpo.registry import HyperparameterConfig, RLParameter
    from agilerl_amd.hpo.tournament import TournamentSelection
    from agilerl_amd.training import train_bandits
    from agilerl_amd.utils import create_population

    env = _env()
    hp = HyperparameterConfig(lr=RLParameter(min=1e-4, max=1e-2), batch_size=RLParameter(min=8, max=32, dtype=int),
                              learn_step=RLParameter(min=1, max=4, dtype=int))
    np.random.seed(0)
    torch.manual_seed(0)
    pop = create_population("NeuralTS", None, {"BATCH_SIZE": 8}, env.observation_space, env.action_space,
                            hp_config=hp, population_size=2)
    assert all(a.device.type == "cuda" and a.sigma_inv.is_cuda for a in pop)
    memory = ReplayBuffer(500)
    muts = Mutations(no_mutation=0.1, architecture=0.3, new_layer_prob=0.2, parameters=0.3, activation=0, rl_hp=0.3,
                     rand_seed=1)
    ckpt = str(tmp_path / "pop")
    pop, fits = train_bandits(env, "synthetic", "NeuralTS", pop, memory, max_steps=64, episode_steps=16, evo_steps=32,
                              eval_steps=8, eval_loop=1, tournament=TournamentSelection(2, True, 2, 1), mutation=muts,
                              checkpoint=32, checkpoint_path=ckpt, save_elite=True, elite_path=str(tmp_path / "elite"),
                              verbose=False)
    assert len(pop) == 2 and len(fits) == 4 and all(len(f) == 2 and np.isfinite(f).all() for f in fits)
    assert len(memory) == 128 and memory.storage["obs"].shape[1:] == (24,)
    for agent in pop:
        assert agent.steps[-1] == 64 and len(agent.regret) == 65 and int(agent.ts_counter) >= 16
        assert agent.sigma_inv.shape == (agent.numel, agent.numel) and torch.isfinite(agent.sigma_inv).all()
        assert all(torch.isfinite(p).all() for p in agent.actor.parameters())
    files = sorted(os.path.basename(f) for f in glob.glob(ckpt + "_*.pt"))
    assert files == ["pop_0_32.pt", "pop_0_64.pt", "pop_1_32.pt", "pop_1_64.pt"]
    loaded = NeuralTS.load(f"{ckpt}_0_64.pt")
    assert torch.equal(loaded.sigma_inv, pop[0].sigma_inv) and int(loaded.ts_counter) == int(pop[0].ts_counter)
    assert os.path.exists(str(tmp_path / "elite.pt"))

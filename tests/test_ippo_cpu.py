"""IPPO without a GPU: the twin (tests/ippo_twin.py) against goldens from the
reference's own ``_learn_individual`` (tests/golden/gen_ippo_golden.py), the
(t, agent, env) assembly order, ``get_action``'s disassembly with the group
forward stubbed, and the argument validation of agx_ippo_gae and of
agx_ppo_learn_args.adv_norm_minibatch, which happens before any HIP call.

Bounds.  The twin and the reference both evaluate in float32; META_ippo.json
records the reference's error against a float64 evaluation of the same
formulas (err_ref_*).  The twin's own float32 error is of that size too (the
same operations, sums in another order), so the two differ by at most about
twice err_ref; the tests allow 4 x err_ref.
"""

import ctypes
import json
import os

import numpy as np
import pytest
import torch

import ippo_twin as twin

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLD, "META_ippo.json")))
LEARN_CASES = ["ippo_even", "ippo_ragged", "ippo_box"]
MULT = 4.0


def _load(name):
    return dict(np.load(os.path.join(GOLD, f"{name}.npz")))


def _spec(case):
    from agilerl_amd.population.nets import ActorCriticSpec, GaussianActorCriticSpec

    kw = dict(obs_dim=case["obs"], n_actions=case["actions"], encoder_hidden=[16], latent_dim=8, actor_hidden=[8],
              critic_hidden=[8], share_encoders=False, encoder_name="actor_encoder")
    return GaussianActorCriticSpec(action_std_init=-0.5, **kw) if case["box"] else ActorCriticSpec(**kw)


def _rows(rec, key, k, T, tail=()):
    from agilerl_amd.algorithms.ippo import assemble_rows

    return assemble_rows({j: rec[f"{key}_{j}"] for j in range(k)}, list(range(k)), T, tail)


@pytest.mark.parametrize("name", sorted(META["cases"]))
def test_gae_twin_bit_exact(name):
    """Advantages and returns of every golden case, k = 2 included, bit for bit."""
    rec, case = _load(name), META["cases"][name]
    T, k = case["T"], case["k"]
    adv, ret = twin.gae_f32(_rows(rec, "rew", k, T), _rows(rec, "done", k, T), _rows(rec, "val", k, T),
                            rec["next_value"], _rows(rec, "next_done", k, None), float(rec["gamma"]),
                            float(rec["gae_lambda"]))
    assert adv.dtype == np.float32 and adv.shape == (T, case["N"] * k)
    assert np.array_equal(adv.view(np.uint32), rec["adv"].view(np.uint32))
    assert np.array_equal(ret.view(np.uint32), rec["ret"].view(np.uint32))


@pytest.mark.parametrize("name", LEARN_CASES)
def test_learn_twin_matches_reference(name):
    rec, case, err = _load(name), META["cases"][name], META["errors"][name]
    assert int(rec["ref_failed"]) == 0
    T, D, A, box = case["T"], case["obs"], case["actions"], case["box"]
    S = T * case["N"]
    hp = {k: META["hp"][k] for k in ("lr", "clip", "ent", "vf", "max_norm")}
    z = np.zeros_like(rec["params"])
    p, m, v, steps, loss = twin.learn(
        _spec(case), rec["params"], z, z, 0, _rows(rec, "obs", 1, T, (D,)).reshape(S, D),
        _rows(rec, "act", 1, T, (A,) if box else ()).reshape(S, *([A] if box else [])),
        _rows(rec, "logp", 1, T).reshape(S), rec["adv"].reshape(-1), rec["ret"].reshape(-1),
        _rows(rec, "val", 1, T).reshape(S), rec["perms"], int(rec["batch"]), how="torch", **hp)
    d = dict(params=np.abs(p.numpy() - rec["params_after"]).max(), moments=np.abs(m.numpy() - rec["exp_avg"]).max(),
             moments2=np.abs(v.numpy() - rec["exp_avg_sq"]).max(), loss=abs(loss - float(rec["loss"])))
    print(name, {k: (float(x), err[f"err_ref_{k}"]) for k, x in d.items()})
    assert steps == int(rec["steps"]) == case["epochs"] * -(-S // int(rec["batch"]))
    assert err["update"] > 1e3 * err["err_ref_params"]  # the update dwarfs the bound
    for k, x in d.items():
        assert x <= MULT * err[f"err_ref_{k}"], (k, x, err[f"err_ref_{k}"])


def test_one_row_case():
    """T = N = k = 1, batch 2: the reference fails on its own squeeze (the
    generator records that); by its formulas the one-row minibatch is skipped:
    no update, loss 0, one GAE step."""
    rec, case = _load("ippo_t1"), META["cases"]["ippo_t1"]
    assert int(rec["ref_failed"]) == 1
    z = np.zeros_like(rec["params"])
    p, m, v, steps, loss = twin.learn(
        _spec(case), rec["params"], z, z, 0, rec["obs_0"].reshape(1, -1), rec["act_0"].reshape(1),
        rec["logp_0"].reshape(1), rec["adv"].reshape(-1), rec["ret"].reshape(-1), rec["val_0"].reshape(1),
        rec["perms"], int(rec["batch"]), lr=1e-3, clip=0.2, ent=0.01, vf=0.5, max_norm=0.5)
    assert steps == 0 and loss == 0.0 and np.array_equal(p.numpy(), rec["params"])
    f = np.float32
    r, d, v0 = f(rec["rew_0"][0, 0]), f(rec["next_done_0"][0]), f(rec["val_0"][0, 0])
    delta = f(f(r + f(f(f(0.99) * f(rec["next_value"][0])) * f(f(1) - d))) - v0)
    assert rec["adv"][0, 0] == delta and rec["ret"][0, 0] == f(delta + v0)


def test_reference_row_order_defect_is_recorded():
    """The generator found the reference pairing a k = 2 group's states with
    other transitions' log-probs from the fourth row on (T = 5, N = 3)."""
    assert META["defect_first_mismatch_row"] == 3


def test_normalize_f64_rounds_like_torch_within_float32():
    a = torch.tensor(np.random.default_rng(0).standard_normal(12).astype(np.float32))
    x, y = twin.normalize(a, "torch").numpy(), twin.normalize(a, "f64").numpy()
    np.testing.assert_allclose(x, y, rtol=4e-6, atol=1e-7)
    np.testing.assert_allclose(y, twin.normalize_f64(a.numpy()).astype(np.float32), rtol=0, atol=0)


# ---- assembly order ---------------------------------------------------------------
AGENTS = ["speaker_0", "listener_0", "listener_1"]


def _structure():
    from agilerl_amd.algorithms.ippo import IPPO
    from agilerl_amd.envs import Box, Discrete

    dims = {"speaker_0": (3, 3), "listener_0": (11, 5), "listener_1": (11, 5)}
    agent = object.__new__(IPPO)
    agent._setup_agents({a: Box(-np.inf, np.inf, (o,)) for a, (o, _) in dims.items()},
                        {a: Discrete(n) for a, (_, n) in dims.items()}, None)
    agent.training = True
    return agent


def test_group_structure():
    agent = _structure()
    assert agent.agent_ids == AGENTS and agent.shared_agent_ids == ["speaker", "listener"]
    assert dict(agent.grouped_agents) == {"speaker": ["speaker_0"], "listener": ["listener_0", "listener_1"]}
    assert agent.has_grouped_agents() and list(agent.observation_space) == ["speaker", "listener"]
    assert agent.get_network_id("listener_1") == "listener"


def test_assembly_rows_are_t_agent_env():
    """A tagged k = 2 tuple: every array's row t (agent j, env n) sits at
    [t, j N + n], the per-env arrays at [j N + n]."""
    from agilerl_amd.algorithms.ippo import assemble_rows

    T, N, D = 5, 3, 4
    tag = lambda j: (100 * np.arange(T)[:, None] + 10 * j + np.arange(N)[None, :]).astype(np.float32)  # noqa: E731
    members = ["listener_0", "listener_1"]
    flat = {a: tag(j) for j, a in enumerate(members)}
    lists = {a: [row for row in tag(j)] for j, a in enumerate(members)}  # the training loop's per-step lists
    wide = {a: np.repeat(tag(j)[:, :, None], D, axis=2) for j, a in enumerate(members)}
    want = np.concatenate([tag(0), tag(1)], axis=1)
    for src in (flat, lists, {a: torch.tensor(x) for a, x in flat.items()}, {a: x[..., None] for a, x in flat.items()}):
        got = assemble_rows(src, members, T)
        assert got.shape == (T, 2 * N) and np.array_equal(got, want)
    got = assemble_rows(wide, members, T, (D,))
    assert got.shape == (T, 2 * N, D) and all(np.array_equal(got[..., d], want) for d in range(D))
    last = {a: tag(j)[-1] for j, a in enumerate(members)}
    assert np.array_equal(assemble_rows(last, members, None), want[-1])
    assert np.array_equal(assemble_rows({a: wide[a][-1] for a in members}, members, None, (D,))[:, 0], want[-1])


def test_get_action_disassembly_with_stubbed_forward():
    agent = _structure()
    N, seen = 4, {}

    def step(net_id, obs, mask, sample=True):
        seen[net_id] = (obs.copy(), None if mask is None else mask.copy())
        M = obs.shape[0]
        ids = np.arange(M)
        return ids.astype(np.int64), -ids.astype(np.float32), 10.0 + ids.astype(np.float32), obs[:, 0].copy()

    agent._group_step = step
    obs = {a: np.full((N, d), i, np.float32) + np.arange(N, dtype=np.float32)[:, None] / 10
           for i, (a, d) in enumerate(zip(AGENTS, (3, 11, 11)))}
    mask = {a: {"action_mask": np.eye(5, dtype=np.int8)[[i] * N]} for i, a in enumerate(AGENTS)}
    mask["speaker_0"] = {}
    action, logp, ent, value = agent.get_action(obs, mask)
    assert list(action) == AGENTS
    # agent-major batch: listener_0's envs, then listener_1's
    assert np.array_equal(seen["listener"][0], np.concatenate([obs["listener_0"], obs["listener_1"]]))
    assert seen["speaker"][1] is None and seen["listener"][1].shape == (2 * N, 5)
    assert np.array_equal(seen["listener"][1][:N], mask["listener_0"]["action_mask"])
    assert np.array_equal(action["listener_0"], np.arange(N)) and np.array_equal(action["listener_1"], N + np.arange(N))
    assert action["listener_1"].dtype == np.int64 and action["listener_1"].shape == (N,)
    assert np.array_equal(logp["listener_1"], -(N + np.arange(N, dtype=np.float32)))
    assert np.array_equal(ent["speaker_0"], 10.0 + np.arange(N, dtype=np.float32))
    for a in AGENTS:
        assert np.array_equal(value[a], obs[a][:, 0]) and value[a].shape == (N,)
    with pytest.raises(NotImplementedError, match="env_defined_actions"):
        agent.get_action(obs, {"speaker_0": {"env_defined_actions": np.zeros(N)}})
    with pytest.raises(AssertionError, match="action masks"):
        agent.get_action(obs, {"listener_0": mask["listener_0"], "listener_1": {}})


def test_unsupported_configurations_raise():
    from agilerl_amd.algorithms.ippo import IPPO
    from agilerl_amd.envs import Box, Discrete

    obs = {"a_0": Box(-1, 1, (3,)), "a_1": Box(-1, 1, (4,))}
    act = {"a_0": Discrete(2), "a_1": Discrete(2)}
    with pytest.raises(AssertionError, match="same observation space"):
        object.__new__(IPPO)._setup_agents(obs, act, None)
    with pytest.raises(NotImplementedError, match="vector observations"):
        object.__new__(IPPO)._setup_agents({"a_0": Box(0, 1, (3, 8, 8))}, {"a_0": Discrete(2)}, None)
    with pytest.raises(NotImplementedError, match="custom actor"):
        IPPO({"a_0": Box(-1, 1, (3,))}, {"a_0": Discrete(2)}, actor_networks=object(), critic_networks=object())
    with pytest.raises(NotImplementedError, match="ROCm device"):
        IPPO({"a_0": Box(-1, 1, (3,))}, {"a_0": Discrete(2)}, device="cpu")


# ---- argument validation, no GPU work ------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from agilerl_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load(require_gpu=False)


def _seg(M=4, **null):
    from agilerl_amd.kernels import IppoGaeSegment

    s = IppoGaeSegment(*([0x1000] * 7), M)
    for k in null:
        setattr(s, k, None)
    return s


def test_ippo_gae_argument_checks(lib):
    from agilerl_amd.kernels import IppoGaeSegment

    def call(segs, n, T):
        arr = (IppoGaeSegment * max(1, len(segs)))(*segs)
        return lib.agx_ippo_gae(ctypes.cast(arr, ctypes.c_void_p), n, T, 0.99, 0.95, None)

    for name in ("rewards", "dones", "values", "next_value", "next_done", "advantages", "returns"):
        assert call([_seg(), _seg(**{name: True})], 2, 8) == -1
        assert b"segment 1: null pointer" in lib.agx_last_error()
    assert call([_seg()], 1, 0) == -1 and b"T=0" in lib.agx_last_error()
    assert call([_seg()], 1, -3) == -1
    assert call([_seg(M=-1)], 1, 8) == -1 and b"negative" in lib.agx_last_error()
    assert call([_seg()] * 9, 9, 8) == -1 and b"max 8" in lib.agx_last_error()
    assert lib.agx_ippo_gae(None, 1, 8, 0.99, 0.95, None) == -1
    assert call([_seg()], -1, 8) == -1
    # nothing to compute: no segments, or only M = 0 segments (their pointers are not read)
    assert lib.agx_ippo_gae(None, 0, 8, 0.99, 0.95, None) == 0
    assert call([IppoGaeSegment()] * 8, 8, 8) == 0


def _learn_args(S, batch, **kw):
    from agilerl_amd.population.learner import AgxPPOLearnArgs

    a = AgxPPOLearnArgs()
    a.P, a.S, a.epochs, a.batch = 1, S, 2, batch
    for name in ("params", "exp_avg", "exp_avg_sq", "adam_step", "lr", "obs", "actions", "old_logp", "adv", "ret",
                 "old_value", "perms", "loss_out"):
        setattr(a, name, 0x1000)
    a.adv_norm_minibatch = 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _graph_learners(lib):
    """(name, call(args) -> rc) for the four graph learners on small valid descriptors."""
    from agilerl_amd.population.nets import (ActorCriticSpec, GaussianActorCriticSpec, MultiBinaryActorCriticSpec,
                                            MultiDiscreteActorCriticSpec)
    from agilerl_amd.population.learner import graph_descriptor

    kw = dict(obs_dim=5, encoder_hidden=[16], latent_dim=8, actor_hidden=[8], critic_hidden=[8],
              share_encoders=False, encoder_name="actor_encoder")
    cat = ActorCriticSpec(n_actions=3, **kw)
    gauss = GaussianActorCriticSpec(n_actions=2, **kw)
    multi = MultiDiscreteActorCriticSpec(n_actions=5, nvec=(2, 3), **kw)
    bern = MultiBinaryActorCriticSpec(n_actions=3, **kw)
    out, ws = [], 0x1000
    d = graph_descriptor(cat)
    out.append(("agx_ppo_learn_graph", lambda a, d=d: lib.agx_ppo_learn_graph(ctypes.byref(d), ctypes.byref(a), ws, None)))
    d = gauss.learn_descriptor_head()
    out.append(("agx_ppo_learn_gauss_graph",
                lambda a, d=d: lib.agx_ppo_learn_gauss_graph(ctypes.byref(d), gauss.log_std, ctypes.byref(a), ws, None)))
    d, mh = multi.learn_descriptor_head(), multi.multi_head()
    out.append(("agx_ppo_learn_multi_graph",
                lambda a, d=d: lib.agx_ppo_learn_multi_graph(ctypes.byref(d), mh, ctypes.byref(a), ws, None)))
    d = bern.learn_descriptor_head()
    out.append(("agx_ppo_learn_bern_graph", lambda a, d=d: lib.agx_ppo_learn_bern_graph(ctypes.byref(d), ctypes.byref(a), ws, None)))
    assert all(x is not None for x in (graph_descriptor(cat), gauss.learn_descriptor_head(),
                                       multi.learn_descriptor_head(), bern.learn_descriptor_head()))
    return out


def test_adv_norm_minibatch_argument_checks(lib):
    """Every rejection comes before any launch (the pointers are dummies), on
    all four graph learners, with the entry point named in the message."""
    for name, call in _graph_learners(lib):
        assert call(_learn_args(64, 8, adv_stats=0x1000)) == -1
        msg = lib.agx_last_error()
        assert name.encode() in msg and b"adv_stats must be NULL" in msg
        for S, batch in ((65, 8), (9, 4), (64, 1), (1, 8)):  # S % batch == 1; one-row minibatches; S = 1
            assert call(_learn_args(S, batch)) == -1, (name, S, batch)
            assert b"one-row minibatch" in lib.agx_last_error()
        assert call(_learn_args(64, 8, batch_per_agent=0x1000)) == -3
        assert name.encode() in lib.agx_last_error() and b"batch_per_agent" in lib.agx_last_error()


def test_adv_norm_minibatch_on_compiled_shapes_is_unsupported(lib):
    from agilerl_amd.population.learner import AgxPPONet

    net = AgxPPONet()
    assert lib.agx_ppo_learn(ctypes.byref(net), ctypes.byref(_learn_args(64, 8)), 0x1000, None) == -3
    assert b"agx_ppo_learn: adv_norm_minibatch is not supported" in lib.agx_last_error()


def test_learn_args_mirror_has_the_trailing_field():
    from agilerl_amd.population.learner import AgxPPOLearnArgs

    names = [f[0] for f in AgxPPOLearnArgs._fields_]
    assert names[-1] == "adv_norm_minibatch" and names[-2] == "skip_if_set"
    assert AgxPPOLearnArgs.adv_norm_minibatch.size == 4
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "agx.h")).read()
    body = hdr[hdr.index("typedef struct agx_ppo_learn_args"):hdr.index("} agx_ppo_learn_args;")]
    assert body.rstrip().endswith("int32_t adv_norm_minibatch;")

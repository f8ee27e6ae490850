"""Generate the bandit golden vectors from the reference's OWN
``NeuralUCB.get_action``.

Test infrastructure only, in the manner of gen_cqn_golden.py (the import
stubs and path loader are gen_golden.py's): the reference source file is
executed in place, nothing of it is copied, and only seeded inputs and the
outputs the reference produced are written — ``bandit_*.npz`` and
``META_bandit.json`` beside this script.  Skips cleanly when the reference
checkout is absent.

Reference function exercised (path relative to the reference checkout):
  * agilerl/algorithms/neural_ucb_bandit.py:185-259   NeuralUCB.get_action (the per-arm backward passes,
                                                      the two batched matmuls, the numpy / numpy.ma argmax,
                                                      the Sherman-Morrison update)
  * agilerl/wrappers/learning.py:40-92                BanditEnv (``bandit_env.npz``: reset and steps under
                                                      random.seed on a small seeded DataFrame)

``get_action`` runs unbound on an ``object.__new__`` stand-in whose ``actor``
is a small seeded torch net — obs -> E -> L -> H -> 1, ReLU between, the shape
of a ValueNetwork with one encoder layer, so the CPU agent test can load its
weights — ending in a real ``nn.Linear(H, 1)`` (the exploration layer), whose
``optimizer.zero_grad`` clears that layer's grads and whose
``preprocess_observation`` is the identity.  T consecutive steps per case;
per step the context, h (the exploration layer's input), mu, the mask, the
action, sigma_inv after the step and ``action_values`` (captured by wrapping
the loaded module's ``np.argmax``) are recorded.

META_bandit.json records, per case and step, the error of the reference's
float32 ``action_values`` / quadratic forms / ``sigma_inv`` against a float64
evaluation of the same formula on the same inputs — the step's float32 h, mu
and the float32 sigma_inv the reference held before it (``err_ref_scores``,
``err_ref_quad``, ``err_ref_sigma``: max abs over elements; the float32
quadratic forms from the torch ops the reference's line calls) — and the
float64 gap between the best and second-best legal score.  The generator asserts gap >= 64 x
err_ref_scores at every step and takes the next seed when a step misses it, so
no fixture can flip an action by rounding.  The single-row-context case has
every arm on identical inputs: its scores are equal by construction, the
first legal index wins in every arithmetic, and its gap is recorded as null.

Usage:  python tests/golden/gen_bandit_golden.py --ref <reference checkout>
"""

from __future__ import annotations

import argparse
import json
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gen_golden import _install_stubs, _load, _stub  # noqa: E402

OBS, ENC, LATENT = 6, 12, 8
GAMMA, LAMB = 1.0, 1.0
# name -> (A, H, T, mask kind, single-row context)
CASES = {
    "bandit_0": (1, 1, 4, None, False),
    "bandit_1": (3, 32, 64, None, False),
    "bandit_2": (10, 32, 64, "random", False),
    "bandit_3": (4, 63, 16, None, False),
    "bandit_4": (5, 64, 16, "random", False),
    "bandit_5": (65, 32, 8, None, False),
    "bandit_single": (4, 32, 8, "not_first", True),  # the repeated-g branch
    "bandit_onehot": (6, 32, 16, "worst", False),    # one legal arm; the masked-out arms hold the top score
}


class _NumpyProxy:
    """The module's ``np`` with ``argmax`` recording its argument."""

    def __init__(self, seen: list):
        self._seen = seen

    def __getattr__(self, name):
        return getattr(np, name)

    def argmax(self, a, *args, **kw):
        self._seen.append(np.array(np.ma.getdata(a), copy=True))
        return np.argmax(a, *args, **kw)


def _net(H: int, seed: int) -> torch.nn.Sequential:
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(OBS, ENC), torch.nn.ReLU(), torch.nn.Linear(ENC, LATENT),
                              torch.nn.ReLU(), torch.nn.Linear(LATENT, H), torch.nn.ReLU(), torch.nn.Linear(H, 1))
    with torch.no_grad():  # lively features and well separated scores
        for m in net:
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(2.0)
                m.bias.uniform_(-0.5, 0.5)
    return net


def _f64_step(S, g, mu, mask, gamma):
    """One step of the formula in float64 -> (quad, scores, action, gap, S')."""
    quad = np.einsum("ki,ij,kj->k", g, S, g)
    scores = mu + gamma * np.sqrt(quad)
    legal = np.ones(len(mu), bool) if mask is None else mask == 1
    action = int(np.argmax(scores)) if mask is None else int(np.argmax(np.ma.array(scores, mask=1 - mask)))
    top = np.sort(scores[legal])[::-1]
    gap = float(top[0] - top[1]) if len(top) > 1 else float("inf")
    v = g[action][:, None]
    S = S - (S @ v @ v.T @ S) / (1.0 + v.T @ S @ v)
    return quad, scores, action, gap, S


def _run(mod, A: int, H: int, T: int, mask_kind, single: bool, seed: int):
    net = _net(H, seed)
    layer = net[-1]
    seen: list = []
    mod.np = _NumpyProxy(seen)

    class _Opt:
        def zero_grad(self):
            layer.weight.grad = None
            layer.bias.grad = None

    fake = object.__new__(mod.NeuralUCB)
    fake.actor, fake.exp_layer, fake.optimizer = net, layer, _Opt()
    fake.numel, fake.action_dim, fake.gamma = H + 1, A, GAMMA
    fake.device, fake.accelerator = "cpu", None
    fake.sigma_inv = LAMB * torch.eye(H + 1)
    fake.preprocess_observation = lambda x: x

    rng = np.random.default_rng(seed)
    rec = {k: [] for k in ("context", "h", "mu", "mask", "action", "sigma_inv", "action_values")}
    errs = {k: [] for k in ("err_ref_scores", "err_ref_quad", "err_ref_sigma", "gap")}
    beaten = 0
    for _ in range(T):
        ctx = torch.from_numpy(rng.standard_normal((1 if single else A, OBS)).astype(np.float32))
        with torch.no_grad():
            h = net[:-1](ctx)
            mu = net(ctx).reshape(-1)
        if single:
            h, mu = h.repeat(A, 1), mu.repeat(A)
        g32 = torch.cat([h, torch.ones(A, 1)], dim=1)
        with torch.no_grad():  # the float32 quadratic forms, by the ops of neural_ucb_bandit.py:239-242
            quad32 = torch.matmul(torch.matmul(g32[:, None, :], fake.sigma_inv), g32[:, :, None])[:, 0, :].squeeze(-1)
        g64, mu64 = g32.numpy().astype(np.float64), mu.numpy().astype(np.float64)
        S64 = fake.sigma_inv.numpy().astype(np.float64)  # the step's own input, as the reference holds it
        mask = None
        if mask_kind == "random":
            mask = (rng.random(A) < 0.6).astype(np.int64)
            mask[rng.integers(0, A)] = 1
        elif mask_kind == "not_first":
            mask = np.ones(A, np.int64)
            mask[0] = 0
        elif mask_kind == "worst":
            pre = mu64 + GAMMA * np.sqrt(np.einsum("ki,ij,kj->k", g64, S64, g64))
            mask = np.zeros(A, np.int64)
            mask[int(np.argmin(pre))] = 1
            beaten += int(np.argmax(pre) != np.argmin(pre))
        quad64, scores64, action64, gap, S64 = _f64_step(S64, g64, mu64, mask, GAMMA)  # S64: after the step
        action = int(fake.get_action(ctx, action_mask=mask))
        values = seen[-1].astype(np.float32)
        err_scores = float(np.max(np.abs(values.astype(np.float64) - scores64)))
        if action != action64 or (not single and not gap >= 64 * err_scores):
            return None  # a near-tie: the next seed
        rec["context"].append(ctx.numpy())
        rec["h"].append(h.numpy())
        rec["mu"].append(mu.numpy())
        rec["mask"].append(np.ones(A, np.uint8) if mask is None else mask.astype(np.uint8))
        rec["action"].append(action)
        rec["sigma_inv"].append(fake.sigma_inv.numpy().copy())
        rec["action_values"].append(values)
        errs["err_ref_scores"].append(err_scores)
        errs["err_ref_quad"].append(float(np.max(np.abs(quad32.numpy().astype(np.float64) - quad64))))
        errs["err_ref_sigma"].append(float(np.max(np.abs(fake.sigma_inv.numpy().astype(np.float64) - S64))))
        errs["gap"].append(gap if np.isfinite(gap) and not single else None)  # null: no second legal arm / equal arms
    if mask_kind == "worst" and beaten == 0:
        return None
    out = {k: np.stack(v) for k, v in rec.items() if k != "action"}
    out["action"] = np.asarray(rec["action"], np.int64)
    out["masked"] = np.bool_(mask_kind is not None)
    out["gamma"], out["lamb"], out["seed"] = np.float64(GAMMA), np.float64(LAMB), np.int64(seed)
    for i, p in enumerate(net.parameters()):
        out[f"param_{i}"] = p.detach().numpy().copy()
    return out, errs


def _bandit_env(ref: str) -> dict:
    """The reference's own BanditEnv (wrappers/learning.py:40-92) on a small
    seeded DataFrame under random.seed: contexts and rewards of a reset and 12
    steps with a fixed arm sequence."""
    import random

    import pandas as pd

    sys.modules["gymnasium"].utils = _stub("gymnasium.utils")  # the file's Skill class derives from gym.utils.*
    mod = _load(ref, "agilerl.wrappers.learning", "agilerl/wrappers/learning.py")
    rng = np.random.default_rng(77)
    features = rng.standard_normal((9, 3)).round(3)
    targets = np.array(["b", "a", "c", "a", "b", "b", "c", "a", "c"])
    env = mod.BanditEnv(pd.DataFrame(features), pd.DataFrame(targets))
    random.seed(1234)
    arms = rng.integers(0, env.arms, 12)
    contexts, rewards = [env.reset()], []
    for k in arms:
        ctx, r = env.step(int(k))
        contexts.append(ctx)
        rewards.append(r)
    return dict(features=features, targets=targets, seed=np.int64(1234), arms=arms.astype(np.int64),
                n_arms=np.int64(env.arms), context_dim=np.int64(env.context_dim[0]), contexts=np.stack(contexts),
                rewards=np.asarray(rewards, np.float64))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=None, help="the reference checkout (the directory that holds agilerl/)")
    args = ap.parse_args()
    ref = args.ref
    if ref is None or not os.path.isdir(os.path.join(ref, "agilerl")):
        print("reference checkout not present; nothing generated")
        return
    torch.set_num_threads(1)
    _install_stubs()
    _stub("agilerl.utils.evolvable_networks")
    mod = _load(ref, "agilerl.algorithms.neural_ucb_bandit", "agilerl/algorithms/neural_ucb_bandit.py")

    errors: dict[str, dict] = {}
    shapes: dict[str, list] = {}
    for k, (name, (A, H, T, mask_kind, single)) in enumerate(CASES.items()):
        for seed in range(500 + 20 * k, 520 + 20 * k):
            got = _run(mod, A, H, T, mask_kind, single, seed)
            if got is not None:
                break
        else:
            raise SystemExit(f"{name}: no seed in range keeps every step's gap above 64 x err_ref_scores")
        rec, errors[name] = got
        shapes[name] = [A, H, T, mask_kind, single]
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < (1 << 20), f"{name}: {os.path.getsize(path)} bytes"
    np.savez_compressed(os.path.join(HERE, "bandit_env.npz"), **_bandit_env(ref))
    meta = {"generator": "tests/golden/gen_bandit_golden.py", "torch": torch.__version__, "numpy": np.__version__,
            "python": sys.version.split()[0], "groups": sorted(errors), "shapes": shapes,
            "net": {"obs": OBS, "encoder": ENC, "latent": LATENT}, "errors": errors,
            "errors_yardstick": "the reference's float32 action_values, quadratic forms and sigma_inv against the "
                                "same formula in float64 numpy on the step's own inputs (its float32 h and mu, the "
                                "float32 sigma_inv the reference held before the step); gap: best minus second-best "
                                "legal float64 score",
            "reference_lines": {"agilerl/algorithms/neural_ucb_bandit.py": "185-259 (NeuralUCB.get_action)",
                                "agilerl/wrappers/learning.py": "40-92 (BanditEnv)"}}
    with open(os.path.join(HERE, "META_bandit.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", len(errors), "fixtures")


if __name__ == "__main__":
    main()

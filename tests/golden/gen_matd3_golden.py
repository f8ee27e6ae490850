"""Generate the MATD3 golden vectors from the reference's OWN ``learn_individual``.

Test infrastructure only, in the manner of gen_td3_golden.py (the import stubs
and path loader are gen_golden.py's): the reference source file is executed in
place, nothing of it is copied, and only seeded inputs and the outputs the
reference produced are written — ``matd3_0..2.npz``, ``matd3_nan.npz`` and
``META_matd3.json`` beside this script.  Skips cleanly when the reference
checkout is absent.

Reference function exercised (path relative to the reference checkout):
  * agilerl/algorithms/matd3.py:786-926   MATD3.learn_individual (torch.min of the two target
                                          critics, the NaN rules — reward NaN -> 0, done NaN -> 1
                                          then uint8 —, y_j, the two MSE losses and their gradients)

``learn_individual`` runs unbound on an ``object.__new__`` stand-in whose
critics return fixed tensors; ``criterion`` records y, the two critic
optimizers' ``step`` records dLoss/dQk, and ``learn_counter`` / ``policy_freq``
are set so that the delayed actor branch is skipped.

Usage:  python tests/golden/gen_matd3_golden.py --ref <reference checkout>
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

# (B, gamma, seed); 33: a part-filled wave, 1024: four blocks of 256 rows
CASES = [(64, 0.95, 301), (33, 0.99, 302), (1024, 0.9, 303)]
NAN_CASE = (33, 0.95, 304)  # one NaN in q_next2


def _inputs(B: int, seed: int, nan_target: bool) -> dict:
    rng = np.random.default_rng(seed)
    f = lambda: rng.standard_normal((B, 1)).astype(np.float32)  # noqa: E731
    rec = dict(q1=f(), q2=f(), q_next1=f(), q_next2=f(), r=f())
    d = (rng.random((B, 1)) < 0.2).astype(np.float32)
    rec["r"][rng.random(B) < 0.05] = np.nan
    d[rng.random(B) < 0.05] = np.nan
    # one reward and one done are NaN whatever the draw, and neither in row 1 or 2
    rec["r"][B // 2, 0] = np.nan
    d[B // 3, 0] = np.nan
    d[1, 0] = 2.0  # uint8 arithmetic: 1 - 2 wraps to 255
    d[2, 0] = 0.0
    rec["r"][1:3, 0] = (0.5, -0.25)
    if nan_target:
        rec["q_next2"][2, 0] = np.nan  # a live row (d = 0): y is NaN there
    rec["d"] = d
    return rec


def _run(MATD3, B: int, gamma: float, seed: int, nan_target: bool = False) -> dict:
    rec = _inputs(B, seed, nan_target)
    Q = [torch.tensor(rec[k], requires_grad=True) for k in ("q1", "q2")]
    got: dict = {"y": []}

    class _Opt:
        def __init__(self, k):
            self.k = k

        def zero_grad(self):
            Q[self.k].grad = None

        def step(self):
            got[f"g_q{self.k + 1}"] = Q[self.k].grad.clone()

    class _NoOpt:
        def zero_grad(self):
            raise AssertionError("the actor branch must be skipped")

        step = zero_grad

    class _Crit:
        def __call__(self, q_eval, y):
            got["y"].append(y.detach().clone())
            return torch.nn.functional.mse_loss(q_eval, y)

    fake = object.__new__(MATD3)
    fake.gamma, fake.accelerator, fake.agent_ids = gamma, None, ["a0"]
    fake.get_network_id = lambda agent_id: agent_id
    fake.actors = {"a0": lambda x: torch.zeros(B, 2)}
    fake.critics_1, fake.critics_2 = {"a0": lambda s, a: Q[0]}, {"a0": lambda s, a: Q[1]}
    fake.critic_targets_1 = {"a0": lambda s, a: torch.tensor(rec["q_next1"])}
    fake.critic_targets_2 = {"a0": lambda s, a: torch.tensor(rec["q_next2"])}
    fake.actor_optimizers = {"a0": _NoOpt()}
    fake.critic_1_optimizers, fake.critic_2_optimizers = {"a0": _Opt(0)}, {"a0": _Opt(1)}
    fake.criterion = _Crit()
    fake.learn_counter, fake.policy_freq = {"a0": 0}, 2  # 1 % 2 != 0: the actor branch is skipped
    zeros = lambda k: {"a0": torch.zeros(B, k)}  # noqa: E731
    actor_loss, critic_loss = MATD3.learn_individual(
        fake, "a0", stacked_actions=torch.zeros(B, 2), stacked_next_actions=torch.zeros(B, 2), states=zeros(1),
        next_states=zeros(1), actions=zeros(2), rewards={"a0": torch.tensor(rec["r"])},
        dones={"a0": torch.tensor(rec["d"])})
    assert actor_loss is None and fake.learn_counter == {"a0": 1}
    assert len(got["y"]) == 2 and torch.equal(got["y"][0].nan_to_num(7.0), got["y"][1].nan_to_num(7.0))
    y = got["y"][0].numpy()
    rec.update(gamma=np.float64(gamma), y=y, g_q1=got["g_q1"].numpy(), g_q2=got["g_q2"].numpy(),
               critic_loss=np.float64(critic_loss))

    # the data reach every branch
    assert np.isnan(rec["r"]).any() and np.isnan(rec["d"]).any() and (rec["d"] == 1).any() and (rec["d"] == 0).any()
    if nan_target:
        assert np.isnan(y[2, 0]) and np.isnan(y).sum() == 1 and np.isnan(critic_loss)
    else:
        assert not np.isnan(y).any() and np.isfinite(critic_loss)
        assert (rec["q_next1"] < rec["q_next2"]).any() and (rec["q_next1"] > rec["q_next2"]).any()
        # the d = 2 row: (1 - 2) in uint8 is 255
        nxt = min(rec["q_next1"][1, 0], rec["q_next2"][1, 0])
        assert y[1, 0] == np.float32(0.5) + (np.float32(255.0) * np.float32(gamma)) * nxt
    return rec


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
    _stub("agilerl.networks.actors")
    matd3 = _load(ref, "agilerl.algorithms.matd3", "agilerl/algorithms/matd3.py")

    groups: dict[str, dict] = {}
    for k, (B, gamma, seed) in enumerate(CASES):
        groups[f"matd3_{k}"] = _run(matd3.MATD3, B, gamma, seed)
    groups["matd3_nan"] = _run(matd3.MATD3, *NAN_CASE, nan_target=True)
    for name, rec in groups.items():
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **rec)
    meta = {"generator": "tests/golden/gen_matd3_golden.py", "torch": torch.__version__, "numpy": np.__version__,
            "python": sys.version.split()[0], "groups": sorted(groups),
            "reference_lines": {"agilerl/algorithms/matd3.py": "786-926 (MATD3.learn_individual)"}}
    with open(os.path.join(HERE, "META_matd3.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", len(groups), "fixtures")


if __name__ == "__main__":
    main()

"""Generate the TD3 / DDPG golden vectors from the reference's OWN ``learn``.

Test infrastructure only, in the manner of gen_golden.py (whose import stubs
and path loader it borrows): the reference source files are executed in place,
nothing of them is copied, and only seeded inputs and the outputs the
reference produced are written — ``td3_0..2.npz``, ``ddpg_0..1.npz`` and
``META_td3.json`` beside this script.  Skips cleanly when the reference
checkout is absent.

Reference functions exercised (paths relative to the reference checkout):
  * agilerl/algorithms/td3.py:462-551    TD3.learn (target-policy smoothing, twin-critic TD
                                         target, the two MSE losses and their gradients)
  * agilerl/algorithms/ddpg.py:422-498   DDPG.learn (the same with one critic)
  * agilerl/utils/algo_utils.py:268-291  multi_dim_clamp (loaded, not restated)

``learn`` runs unbound on an ``object.__new__`` stand-in whose critics return
fixed tensors, whose target actor returns a fixed ``mu`` and whose target
critics record the ``next_actions`` they are given; ``criterion`` records y,
the optimizers' ``step`` records dLoss/dQ, and ``learn_counter`` is set so
that the delayed actor branch is skipped.  The reference draws the smoothing
noise in place into the batch's action tensor, so after the call that tensor
holds the raw N(0, policy_noise) draw, which is recorded as ``noise``.

Usage:  python tests/golden/gen_td3_golden.py --ref <reference checkout>
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

POLICY_NOISE = 0.2

# (B, A, gamma, noise_clip, seed); the second DDPG case fills a second block of 256 rows partly
TD3_CASES = [(64, 2, 0.99, 0.3, 201), (33, 1, 0.95, 0.25, 202), (1024, 6, 0.9, 0.3, 203)]
DDPG_CASES = [(64, 2, 0.99, 0.3, 211), (300, 3, 0.97, 0.25, 212)]


def _inputs(B: int, A: int, seed: int, twin: bool) -> dict:
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    # per-dimension bounds that differ across dimensions, inside the actor's [-1, 1]
    low = (-0.9 + 0.1 * np.arange(A)).astype(np.float32)
    high = (0.8 - 0.07 * np.arange(A)).astype(np.float32)
    mu = (1.2 * np.tanh(f(B, A))).astype(np.float32)  # reaches past both bounds
    d = (rng.random((B, 1)) < 0.2).astype(np.float32)
    d[0, 0] = 1.0
    rec = dict(mu=mu, low=low, high=high, q1=f(B, 1), qn1=f(B, 1), r=f(B, 1), d=d)
    if twin:
        rec.update(q2=f(B, 1), qn2=f(B, 1))
    return rec


def _run(cls, mdc, B: int, A: int, gamma: float, noise_clip: float, seed: int, twin: bool) -> dict:
    rec = _inputs(B, A, seed, twin)
    Q = [torch.tensor(rec[k], requires_grad=True) for k in (("q1", "q2") if twin else ("q1",))]
    got: dict = {}

    def critic(k):
        return lambda obs, actions: Q[k]

    def target(k):
        def call(obs, actions):
            got["next_actions"] = actions.detach().clone()
            return torch.tensor(rec[f"qn{k + 1}"])
        return call

    class _Opt:
        def __init__(self, k):
            self.k = k

        def zero_grad(self):
            Q[self.k].grad = None

        def step(self):
            got[f"g_q{self.k + 1}"] = Q[self.k].grad.clone()

    class _Crit:
        def __call__(self, q_eval, y):
            got["y"] = y.detach().clone()
            return torch.nn.functional.mse_loss(q_eval, y)

    fake = object.__new__(cls)
    fake.preprocess_observation = lambda obs: obs
    fake.device, fake.accelerator, fake.gamma = torch.device("cpu"), None, gamma
    fake.actor_target = lambda obs: torch.tensor(rec["mu"])
    fake.action_low, fake.action_high = torch.tensor(rec["low"]), torch.tensor(rec["high"])
    fake.criterion = _Crit()
    fake.learn_counter, fake.policy_freq = 0, 2  # 1 % 2 != 0: the actor branch is skipped
    if twin:
        fake.critic_1, fake.critic_2 = critic(0), critic(1)
        fake.critic_target_1, fake.critic_target_2 = target(0), target(1)
        fake.critic_1_optimizer, fake.critic_2_optimizer = _Opt(0), _Opt(1)
    else:
        fake.critic, fake.critic_target, fake.critic_optimizer = critic(0), target(0), _Opt(0)
    # learn() reads multi_dim_clamp from its module's globals: the reference's own
    assert sys.modules[cls.__module__].multi_dim_clamp is mdc
    action = torch.zeros(B, A)
    torch.manual_seed(seed)
    actor_loss, critic_loss = cls.learn(fake, {"obs": torch.zeros(B, 4), "action": action, "reward": torch.tensor(rec["r"]),
                                               "next_obs": torch.zeros(B, 4), "done": torch.tensor(rec["d"])},
                                        noise_clip=noise_clip, policy_noise=POLICY_NOISE)
    assert actor_loss is None and fake.learn_counter == 1
    noise = action.numpy().copy()  # the in-place draw
    rec.update(noise=noise, noise_clip=np.float64(noise_clip), gamma=np.float64(gamma),
               next_actions=got["next_actions"].numpy(), y=got["y"].numpy(), g_q1=got["g_q1"].numpy(),
               critic_loss=np.float64(critic_loss))
    if twin:
        rec["g_q2"] = got["g_q2"].numpy()

    # the data reach every branch
    mu, low, high = rec["mu"], rec["low"], rec["high"]
    if A > 1:
        assert len(set(low.tolist())) == A and len(set(high.tolist())) == A
    clipped = np.abs(noise) > noise_clip
    s = mu + np.clip(noise, -noise_clip, noise_clip)
    assert clipped.any() and (s < low).any() and (s > high).any()
    assert (~clipped & (s > low) & (s < high)).any()
    assert (rec["next_actions"] == low).any() and (rec["next_actions"] == high).any()
    assert (rec["d"] == 1).any() and (rec["d"] == 0).any()
    if twin:
        assert (rec["qn1"] < rec["qn2"]).any() and (rec["qn1"] > rec["qn2"]).any()
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
    for name in ("agilerl.networks.actors", "agilerl.networks.base", "agilerl.utils.evolvable_networks",
                 "agilerl.modules.dummy", "agilerl.utils.llm_utils"):
        _stub(name)
    sys.modules["agilerl"].HAS_LLM_DEPENDENCIES = False
    au = _load(ref, "agilerl.utils.algo_utils", "agilerl/utils/algo_utils.py")  # the real multi_dim_clamp
    td3 = _load(ref, "agilerl.algorithms.td3", "agilerl/algorithms/td3.py")
    ddpg = _load(ref, "agilerl.algorithms.ddpg", "agilerl/algorithms/ddpg.py")

    groups: dict[str, dict] = {}
    for k, (B, A, gamma, clip, seed) in enumerate(TD3_CASES):
        groups[f"td3_{k}"] = _run(td3.TD3, au.multi_dim_clamp, B, A, gamma, clip, seed, twin=True)
    for k, (B, A, gamma, clip, seed) in enumerate(DDPG_CASES):
        groups[f"ddpg_{k}"] = _run(ddpg.DDPG, au.multi_dim_clamp, B, A, gamma, clip, seed, twin=False)
    for name, rec in groups.items():
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **rec)
    meta = {"generator": "tests/golden/gen_td3_golden.py", "torch": torch.__version__, "numpy": np.__version__,
            "python": sys.version.split()[0], "policy_noise": POLICY_NOISE, "groups": sorted(groups)}
    with open(os.path.join(HERE, "META_td3.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote", len(groups), "fixtures")


if __name__ == "__main__":
    main()

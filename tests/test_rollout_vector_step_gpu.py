"""The vector step of the persistent rollout (ppo_rollout_persistent_kernel)
against one policy-step launch per vector step (ppo_act_kernel, which zeroes
its activations every launch, computes its Gumbel noise inline and stores
in the plain order): bit for bit, at the shapes where a resident step can go
wrong — zero-once activations, noise computed ahead of the release, stale
wide columns of the shared activation buffers, partial workgroups — and the
paths out of the release wait (stop word, abort word) and the one-call host
pacing (agx_host_signal_wait)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# Shape<8,4,2,64,64,0,64,64> (the bench shape) and Shape<8,4,3,64,64,32,32,16>:
# encoder layers 64, 64, 32 and a merged head of 32 + 16 = 48 columns share
# the 64-wide activation buffers, so narrower layers leave wider ones' columns
NETS = {
    "bench": {},
    "mixed_widths": dict(encoder_hidden=[64, 64], latent_dim=32, actor_hidden=[32], critic_hidden=[16]),
}
ROLLOUT = ("obs", "actions", "log_probs", "values", "rewards", "dones")


def _pair(monkeypatch, persistent, P=2, N=40, T=3, net="bench", env_cls=None, **env_kw):
    from agilerl_amd.envs import SyntheticVecEnv
    from agilerl_amd.population.nets import ActorCriticSpec
    from agilerl_amd.population.ppo_pop import PPOPopulation
    from agilerl_amd.population.runner import PopulationRunner

    monkeypatch.setenv("AGX_PERSISTENT_ROLLOUT", "1" if persistent else "0")
    spec = ActorCriticSpec(obs_dim=8, n_actions=4, **NETS[net])
    pop = PPOPopulation(spec, P, N, learn_step=T * N, batch_size=64, update_epochs=2, device=DEV,
                        seeds=list(range(P)), fused=True, perm_source="device")
    assert pop.T == T and pop.fused_descriptor() is not None  # the compiled kernels, not the runtime-shape ones
    env = (env_cls or SyntheticVecEnv)(P * N, seed=5, p_done=0.3, **env_kw)
    run = PopulationRunner(pop, env)
    assert run.persistent == persistent
    return pop, run


def _rollout_state(pop, run):
    torch.cuda.synchronize()
    st = {name: getattr(pop, name).clone() for name in ROLLOUT}
    st.update(last_obs=run.last_obs.clone(), last_value=run.last_value.clone(), last_done=run.last_done.clone(),
              scores=run.scores.clone(), return_sum=run.ret_sum_env.clone(), episodes=run.episodes_env.clone())
    return st


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        assert torch.equal(a[name], b[name]), f"{what}: {name}"


@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("N", [40, 5])
def test_persistent_vector_step_matches_per_step_launches(monkeypatch, net, N):
    """P = 2 (agent strides), T = 3 (two resident steps and the final scatter
    step), N = 40 (a full and a partial workgroup per agent) or 5 (one partial
    workgroup, 27 dead rows), p_done = 0.3 (the episode accounting fires), two
    launches (the second starts from a fresh zero).  N = 40 runs whole
    iterations (the pipelined pacing, a learn between the launches), N = 5
    collects only (the plain pacing loop)."""
    out = []
    for persistent in (True, False):
        pop, run = _pair(monkeypatch, persistent, N=N, net=net)
        states = []
        for _ in range(2):
            if N == 40:
                run.iteration()
            else:
                run.collect()
                pop.finish_rollout(run.last_obs, run.last_done, run.last_value)
            states.append(_rollout_state(pop, run))
        states[-1]["params"] = pop.params.data.clone()
        states[-1]["advantages"] = pop.advantages.clone()
        if persistent:
            assert int(run.ctl_h.view(torch.int32)[1]) == 0  # no workgroup timed out or aborted
        out.append(states)
    for k, (a, b) in enumerate(zip(*out)):
        _assert_same(a, b, f"launch {k}")
    assert int(out[0][-1]["episodes"].sum()) > 0  # the accounting branch ran
    acts = out[0][-1]["actions"]
    assert int(acts.min()) >= 0 and int(acts.max()) < 4


def test_persistent_evaluation_two_steps_matches_per_step(monkeypatch):
    """evaluate(loop=1, max_steps=2): the launch is sized for more steps than
    are run, so the stop word reaches the release wait in mid launch; fitness
    and the rollout after the pass equal the per-step pass."""
    out = []
    for persistent in (True, False):
        pop, run = _pair(monkeypatch, persistent)
        run.iteration()
        fit = run.evaluate(loop=1, max_steps=2)
        run.iteration()
        st = _rollout_state(pop, run)
        st["params"] = pop.params.data.clone()
        if persistent:
            assert int(run.ctl_h.view(torch.int32)[1]) == 0  # stopped, not timed out
        out.append((fit, st))
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert np.all(np.isfinite(out[0][0]))
    _assert_same(out[0][1], out[1][1], "after the evaluation")


def test_host_exception_at_vector_step_one_leaves_through_the_abort_word(monkeypatch):
    """The env raises in its second step, so the workgroups sit in the release
    wait of vector step 2 when the abort word arrives.  The exception
    propagates, the queued learner skips (parameters, Adam moments and step
    counts bit-unchanged), and a fresh runner's next rollout on that
    population equals the one of a population whose env never raised
    (everything the rollout writes; the minibatch orders of the learns after
    it are not part of this comparison)."""
    from agilerl_amd.envs import SyntheticVecEnv
    from agilerl_amd.population.runner import PopulationRunner

    class Raising(SyntheticVecEnv):
        fail_at = None
        calls = 0

        def step(self, actions, **kw):
            if self.calls == self.fail_at:
                raise RuntimeError("env worker died")
            self.calls += 1
            return super().step(actions, **kw)

    rollouts = []
    for fail in (True, False):
        pop, run = _pair(monkeypatch, True, env_cls=Raising)
        run.iteration()
        torch.cuda.synchronize()
        if fail:
            before = [t.clone() for t in (pop.params.data, pop.opt.exp_avg, pop.opt.exp_avg_sq, pop.opt.steps)]
            run.env.fail_at = run.env.calls + 1  # vector step 1 of the next rollout
            with pytest.raises(RuntimeError, match="env worker died"):
                run.iteration()
            torch.cuda.synchronize()
            pop.check_errors()
            after = (pop.params.data, pop.opt.exp_avg, pop.opt.exp_avg_sq, pop.opt.steps)
            for name, a, b in zip(("params", "exp_avg", "exp_avg_sq", "steps"), before, after):
                assert torch.equal(a, b), name
        fresh = PopulationRunner(pop, SyntheticVecEnv(pop.P * pop.N, seed=11, p_done=0.3))
        assert fresh.persistent
        fresh.collect()
        st = _rollout_state(pop, fresh)
        assert int(fresh.ctl_h.view(torch.int32)[1]) == 0
        rollouts.append(st)
    _assert_same(rollouts[0], rollouts[1], "rollout after the abort")


def test_host_signal_wait_null_ctl_is_an_error():
    from agilerl_amd import _lib

    lib = _lib.load()
    rc = lib.agx_host_signal_wait(None, 1, 1, 1, 1.0)
    assert rc != 0
    assert b"agx_host_signal_wait" in lib.agx_last_error()


def test_host_signal_wait_paces_like_signal_then_wait(monkeypatch):
    """A rollout paced through agx_host_signal_wait equals one paced through
    agx_host_signal + agx_host_wait (the two-call form stands in for the
    one-call entry point on the second runner)."""
    from agilerl_amd import _lib

    lib = _lib.load()
    calls = {"one": 0, "two": 0}
    real = lib.agx_host_signal_wait

    def counted(*a):
        calls["one"] += 1
        return real(*a)

    def two_calls(ctl, seq, nwg, target, timeout_s):
        calls["two"] += 1
        rc = lib.agx_host_signal(ctl, seq)
        return rc if rc else lib.agx_host_wait(ctl, nwg, target, timeout_s)

    out = []
    for fn in (counted, two_calls):
        pop, run = _pair(monkeypatch, True)
        monkeypatch.setattr(lib, "agx_host_signal_wait", fn)
        run.collect()
        pop.finish_rollout(run.last_obs, run.last_done, run.last_value)
        run.iteration()
        monkeypatch.setattr(lib, "agx_host_signal_wait", real)
        st = _rollout_state(pop, run)
        st["params"] = pop.params.data.clone()
        out.append(st)
    assert calls == {"one": 6, "two": 6}  # T = 3 steps of a collect and of an iteration each
    _assert_same(out[0], out[1], "one call against two")

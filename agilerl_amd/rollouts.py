"""Drop-in ``collect_rollouts`` (agilerl/rollouts/on_policy.py:23-203) for an
agx PPO agent: fills the agent's HBM rollout from ``env`` (num_envs envs, or
num_envs x population_size for a population view) and computes the bootstrap
value + GAE, ready for ``agent.learn()``."""

from __future__ import annotations

from .population.runner import PopulationRunner


def collect_rollouts(agent, env, n_steps: int | None = None, last_obs=None, last_done=None, last_scores=None,
                     last_info=None, **_kwargs):
    """-> (completed episode scores, last_obs, last_done, last_scores,
    last_info) as the reference (episode scores of the envs that finished
    during this rollout; the runner carries the env state between calls, so
    the last_* values are returned for the caller's loop and not needed back)."""
    pop = agent.population
    if n_steps is not None and n_steps != pop.T:
        raise ValueError(f"n_steps must equal the rollout capacity ceil(learn_step / num_envs) = {pop.T}")
    runner = getattr(pop, "_runner", None)
    if runner is None or runner.env is not env:
        runner = PopulationRunner(pop, env)
        pop._runner = runner
    runner.reset_episode_stats()
    runner.collect()
    pop.finish_rollout(runner.last_obs, runner.last_done, runner.last_value if runner.last_value_valid else None)
    s = float(runner.episode_return_sum[agent.row].item())
    c = int(runner.episodes[agent.row].item())
    scores = [s / c] * c if c else []
    return scores, runner.last_obs, runner.last_done, None, None


def collect_rollouts_recurrent(agent, env, n_steps: int | None = None, last_obs=None, last_done=None,
                               last_scores=None, last_info=None, **_kwargs):
    """``collect_rollouts_recurrent`` (on_policy.py:23-203, 227-245) for ``PPO(recurrent=True)``: each step's
    hidden state is stored before the step is taken, and goes back to the initial state where the step ended an
    episode.  -> (completed episode scores, obs, done, scores, info) for the caller's next call."""
    import numpy as np

    from .algorithms.ppo_recurrent import reset_hidden_state

    if last_obs is None and last_done is None and last_scores is None and last_info is None:
        obs, info = env.reset()
        scores, done = np.zeros(agent.num_envs), np.zeros(agent.num_envs)
        agent.hidden_state = agent.get_initial_hidden_state(agent.num_envs)
    else:
        obs, done, scores, info = last_obs, last_done, last_scores, last_info
    info = info if isinstance(info, dict) else {}
    n_steps = n_steps or -(agent.learn_step // -agent.num_envs)
    buf = agent.rollout_buffer
    buf.reset()
    box = hasattr(agent.action_space, "low")
    completed = []
    term = np.zeros(agent.num_envs, dtype=bool)
    fused = agent.fused_step_on()
    reset = None  # the previous step's dones: the fused step starts those rows from the zero state itself
    for _ in range(n_steps):
        stored = agent.hidden_state
        mask = info.get("action_mask")
        res = buf.fused_step(agent, obs, mask, stored, reset) if fused else None
        if res is not None:  # slot `pos` holds obs / action / log-prob / value / the state taken; the host adds the rest
            action, log_prob, value, agent.hidden_state = res
        else:
            if reset is not None:
                reset_hidden_state(stored, agent.get_initial_hidden_state(agent.num_envs), reset)
            action, log_prob, _, value, agent.hidden_state = agent.get_action(obs, action_mask=mask,
                                                                              hidden_state=stored)
        env_action = np.clip(action, agent.action_space.low, agent.action_space.high) if box else action
        next_obs, reward, term, trunc, next_info = env.step(env_action)
        ended = np.atleast_1d(np.logical_or(term, trunc))
        reward = np.atleast_1d(reward)
        if res is not None:
            buf.finish_step(reward=reward, done=ended, next_obs=next_obs, action_mask=mask)
        else:
            buf.add(obs=obs, action=action, reward=reward, done=ended, value=np.atleast_1d(value),
                    log_prob=np.atleast_1d(log_prob), next_obs=next_obs, hidden_state=stored, action_mask=mask)
        scores += reward
        done = ended
        reset = None
        if np.any(ended):
            if fused:
                reset = ended
            else:
                reset_hidden_state(agent.hidden_state, agent.get_initial_hidden_state(agent.num_envs), ended)
        obs, info = next_obs, next_info if isinstance(next_info, dict) else {}
        for i in np.flatnonzero(ended):
            completed.append(float(scores[i]))
            agent.scores.append(float(scores[i]))
            scores[i] = 0
    if reset is not None:  # the state handed to the next call is the reset one, as on the torch path
        reset_hidden_state(agent.hidden_state, agent.get_initial_hidden_state(agent.num_envs), reset)
    last_value = agent.bootstrap_value(obs, agent.hidden_state)
    buf.compute_returns_and_advantages(last_value=last_value, last_done=np.atleast_1d(term))
    return completed, obs, done, scores, info

"""Drop-in ``train_multi_agent_on_policy``
(agilerl/training/train_multi_agent_on_policy.py:37-623) for IPPO populations.

Per generation each agent in turn: ``ceil(evo_steps / learn_step)``
collections of ``ceil(learn_step / num_envs)`` vector steps of ``get_action``
(Box actions clipped to the bounds for the env, the unclipped ones stored),
``done`` carried from the previous step's terminations | truncations and
zeroed for every env once an episode of all agents ends, scores summed over
the agents, and one ``agent.learn`` per collection on the 8-tuple of
per-agent dicts; then ``agent.test`` fitness, and tournament selection of
clones and mutations when both objects are given, elite and checkpoint
saving as ``train_multi_agent_off_policy`` does.  No wandb and no accelerator
(DESIGN section 7).  Returns (pop, pop_fitnesses)."""

from __future__ import annotations

import numpy as np

from ..hpo.shard import all_ranks, mutate_population, sync_host_rngs
from ..hpo.sharded import select_population


def _next_done(termination: dict, truncation: dict, vec: bool) -> dict:
    """:316-335: terminations | truncations per agent, NaN where either is NaN."""
    out = {}
    for a in termination:
        term, trunc = termination[a], truncation[a]
        if vec:
            term, trunc = np.asarray(term), np.asarray(trunc)
            ok = ~(np.isnan(term.astype(float)) | np.isnan(trunc.astype(float)))
            res = np.full(ok.shape, np.nan, dtype=float)
            res[ok] = np.logical_or(term[ok], trunc[ok])
            out[a] = res
        else:
            out[a] = np.array([np.logical_or(term, trunc)]).astype(np.int8)
    return out


def train_multi_agent_on_policy(env, env_name: str, algo: str, pop, INIT_HP=None, MUT_P=None,
                                sum_scores: bool = True, swap_channels: bool = False, max_steps: int = 50000,
                                evo_steps: int = 25, eval_steps=None, eval_loop: int = 1, target: float | None = None,
                                tournament=None, mutation=None, checkpoint=None, checkpoint_path=None,
                                overwrite_checkpoints: bool = False, save_elite: bool = False, elite_path=None,
                                wb: bool = False, verbose: bool = True, accelerator=None, wandb_api_key=None,
                                wandb_kwargs=None):
    assert isinstance(algo, str), "'algo' must be the name of the algorithm as a string."
    assert isinstance(max_steps, int), "Number of steps must be an integer."
    assert isinstance(evo_steps, int), "Evolution frequency must be an integer."
    if wb or accelerator is not None:
        raise NotImplementedError("agx train_multi_agent_on_policy: no wandb and no accelerator")
    if save_elite is False and elite_path is not None:
        save_elite = True  # the reference only warns and goes on
    if swap_channels:
        raise NotImplementedError("agx IPPO: vector observations (no image channels to swap)")
    vec = hasattr(env, "num_envs")
    num_envs = env.num_envs if vec else 1
    save_path = (checkpoint_path.split(".pt")[0] if checkpoint_path is not None else f"{env_name}-EvoHPO-{algo}")
    agent_ids = list(pop[0].observation_space.keys())
    pop_fitnesses: list = []
    pop_loss = [{a: [] for a in agent_ids} for _ in pop]
    checkpoint_count = 0
    if mutation is not None:  # pre-training mutation (:193-194)
        pop = mutate_population(mutation, pop, pre_training_mut=True)
    while np.sum([agent.steps[-1] for agent in pop]) < max_steps:
        for agent_idx, agent in enumerate(pop):
            agent.set_training_mode(True)
            obs, info = env.reset()
            scores = np.zeros((num_envs, 1)) if sum_scores else np.zeros((num_envs, len(agent_ids)))
            losses = {a: [] for a in agent_ids}
            steps = 0
            for _ in range(-(evo_steps // -agent.learn_step)):
                ids = agent.agent_ids
                states, actions, log_probs, entropies, rewards, dones, values = ({a: [] for a in ids}
                                                                                 for _ in range(7))
                done = {a: np.zeros(num_envs) for a in ids}
                next_obs, next_done = obs, done
                for _ in range(-(agent.learn_step // -num_envs)):
                    action, log_prob, entropy, value = agent.get_action(obs=obs, infos=info)
                    if not vec:
                        action, log_prob, entropy, value = ({a: x[0] for a, x in d.items()}
                                                            for d in (action, log_prob, entropy, value))
                    clipped = {}
                    for a, act in action.items():  # :249-281: Box actions clipped for the env only
                        space = agent.possible_action_spaces[a]
                        box = hasattr(space, "low") and not hasattr(space, "n") and not hasattr(space, "nvec")
                        clipped[a] = np.clip(act, space.low, space.high) if box else act
                    next_obs, reward, termination, truncation, info = env.step(clipped)
                    r = np.array(list(reward.values())).transpose()
                    r = np.where(np.isnan(r), 0, r)
                    scores += (np.sum(r, axis=-1)[:, None] if vec else np.sum(r, axis=-1)) if sum_scores else r
                    steps += num_envs
                    for a in obs:
                        states[a].append(obs[a])
                        rewards[a].append(reward[a])
                        actions[a].append(action[a])
                        log_probs[a].append(log_prob[a])
                        entropies[a].append(entropy[a])
                        values[a].append(value[a])
                        dones[a].append(done[a])
                    next_done = _next_done(termination, truncation, vec)
                    obs, done = next_obs, next_done
                    for idx, agent_dones in enumerate(zip(*next_done.values())):
                        if all(agent_dones):
                            agent.scores.append(float(scores[idx].item()) if sum_scores else list(scores[idx]))
                            scores[idx].fill(0)
                            if not vec:
                                obs, info = env.reset()
                            done = {a: np.zeros(num_envs) for a in ids}
                loss = agent.learn((states, actions, log_probs, rewards, dones, values, next_obs, next_done))
                for a in agent_ids:
                    losses[a].append(loss[a])
            agent.steps[-1] += steps
            if all(losses[a] for a in agent_ids):
                for a in agent_ids:
                    pop_loss[agent_idx][a].append(float(np.mean([x for x in losses[a] if x is not None])))
        fitnesses = [agent.test(env, swap_channels=swap_channels, max_steps=eval_steps, loop=eval_loop,
                                sum_scores=sum_scores) for agent in pop]
        pop_fitnesses.append(fitnesses)
        if verbose:
            print(f"--- {env_name} {algo}: steps {[a.steps[-1] for a in pop]}, fitness {fitnesses}")
        for agent in pop:
            agent.steps.append(agent.steps[-1])
        if target is not None and all_ranks(np.all(np.greater([np.mean(a.fitness[-10:]) for a in pop], target))) \
                and len(pop[0].steps) >= 100:
            return pop, pop_fitnesses
        if tournament and mutation is not None:  # tournament_selection_and_mutation
            sync_host_rngs()
            elite, pop = select_population(tournament, pop)
            pop = mutate_population(mutation, pop)
            if save_elite and elite is not None:
                elite.save_checkpoint(f"{elite_path.split('.pt')[0]}.pt" if elite_path is not None
                                      else f"{env_name}-elite_{algo}.pt")
            pop_loss = [{a: [] for a in agent_ids} for _ in pop]
        if checkpoint is not None and pop[0].steps[-1] // checkpoint > checkpoint_count:
            for agent in pop:
                agent.save_checkpoint(f"{save_path}_{agent.index}.pt" if overwrite_checkpoints
                                      else f"{save_path}_{agent.index}_{agent.steps[-1]}.pt")
            checkpoint_count += 1
    return pop, pop_fitnesses

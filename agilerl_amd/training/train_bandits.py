"""Drop-in ``train_bandits`` (agilerl/training/train_bandits.py:31-364) for
NeuralUCB / NeuralTS populations on the agx replay buffer.

An episode is ``episode_steps`` env steps of one agent: ``get_action`` on the
context, the env step, one ``memory.add`` and, once the buffer holds a batch,
``learn_step`` updates on fresh samples.  The transition stores
``context[action]`` — the chosen arm's feature row — as ``obs``, which is what
the reference's documentation, demo and tutorials store; its own loop stores
the whole ``[arms, dim]`` context, whose ``[B, arms, 1]`` predictions only
broadcast against ``[B, 1]`` rewards when ``arms`` is 1 or the batch size
(DESIGN.md section 8).  The updates of one env step are enqueued with
``learn_device`` and their losses summed on the device: one read per step,
none per update.

After every agent's episode the population is evaluated with ``agent.test``;
with a tournament AND a mutation object (as the reference) and ``evo_steps``
more steps done, the tournament replaces the population, the elite is saved
when ``save_elite``, and ``mutation.mutation`` mutates it; a population
checkpoint is written every ``checkpoint`` steps to the file names
``train_offline`` uses.  Returns (pop, pop_fitnesses).

Single process only; ``accelerator`` and ``wb`` are ignored, as by the other
loops here.
"""

from __future__ import annotations

import warnings
from datetime import datetime

import numpy as np
import torch

from ..components.sampler import Sampler


def train_bandits(env, env_name: str, algo: str, pop, memory, INIT_HP=None, MUT_P=None, swap_channels: bool = False,
                  max_steps: int = 20000, episode_steps: int = 500, evo_steps: int = 2500, eval_steps: int = 500,
                  eval_loop: int = 1, target: float | None = None, tournament=None, mutation=None, checkpoint=None,
                  checkpoint_path=None, overwrite_checkpoints: bool = False, save_elite: bool = False,
                  elite_path=None, wb: bool = False, verbose: bool = True, accelerator=None, wandb_api_key=None):
    assert isinstance(algo, str), "'algo' must be the name of the algorithm as a string."
    assert isinstance(max_steps, int), "Number of steps must be an integer."
    assert isinstance(evo_steps, int), "Evolution frequency must be an integer."
    if target is not None:
        assert isinstance(target, (float, int)), "Target score must be a float or an integer."
    if checkpoint is not None:
        assert isinstance(checkpoint, int), "Checkpoint must be an integer."
    assert isinstance(wb, bool), "'wb' must be a boolean flag, indicating whether to record run with W&B"
    assert isinstance(verbose, bool), "Verbose must be a boolean."
    if save_elite is False and elite_path is not None:
        warnings.warn("'save_elite' set to False but 'elite_path' has been defined, elite will not "
                      "be saved unless 'save_elite' is set to True.", stacklevel=2)
    if checkpoint is None and checkpoint_path is not None:
        warnings.warn("'checkpoint' set to None but 'checkpoint_path' has been defined, checkpoint will not "
                      "be saved unless 'checkpoint' is defined.", stacklevel=2)
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("train_bandits runs in a single process")
    save_path = (checkpoint_path.split(".pt")[0] if checkpoint_path is not None
                 else f"{env_name}-EvoHPO-{algo}-{datetime.now().strftime('%m%d%Y%H%M%S')}")
    sampler = Sampler(memory=memory)
    if mutation is not None:  # pre-training mutation (:175-177)
        pop = mutation.mutation(pop, pre_training_mut=True)

    pop_loss: list[list[float]] = [[] for _ in pop]
    pop_fitnesses: list[list[float]] = []
    total_steps = 0
    checkpoint_count = 0
    evo_count = 0
    while np.less([agent.steps[-1] for agent in pop], max_steps).all():
        pop_episode_scores = []
        for agent_idx, agent in enumerate(pop):
            score = 0.0
            losses = []
            context = env.reset()
            for _ in range(episode_steps):
                if swap_channels:
                    context = np.moveaxis(np.asarray(context), -1, -3)
                action = agent.get_action(context)
                next_context, reward = env.step(action)
                memory.add({"obs": np.asarray(context[action])[None], "reward": np.asarray([reward], np.float32)})
                if len(memory) >= agent.batch_size:
                    total = torch.zeros((), dtype=torch.float64, device=agent.device)
                    for _ in range(agent.learn_step):
                        total += agent.learn_device(sampler.sample(agent.batch_size))
                    losses.append(float(total.item()) / agent.learn_step)  # the step's one read
                score += float(reward)
                agent.regret.append(agent.regret[-1] + 1 - reward)
                context = next_context
            agent.scores.append(score)
            pop_episode_scores.append(score)
            pop_loss[agent_idx].append(float(np.mean(losses)) if losses else float("nan"))
            agent.steps[-1] += episode_steps
            total_steps += episode_steps
        fitnesses = [agent.test(env, swap_channels=swap_channels, max_steps=eval_steps, loop=eval_loop)
                     for agent in pop]
        pop_fitnesses.append(fitnesses)
        regrets = [agent.regret[-1] for agent in pop]
        for agent in pop:
            agent.steps.append(agent.steps[-1])
        if target is not None and np.all(np.greater([np.mean(a.fitness[-10:]) for a in pop], target)) \
                and len(pop[0].steps) >= 100:
            return pop, pop_fitnesses
        if tournament and mutation is not None and pop[0].steps[-1] // evo_steps > evo_count:
            # tournament_selection_and_mutation (utils.py:1137-1225)
            elite, pop = tournament.select(pop)
            if save_elite and elite is not None:
                elite_save_path = elite_path.split(".pt")[0] if elite_path is not None else f"{env_name}-elite_{algo}"
                elite.save_checkpoint(f"{elite_save_path}.pt")
            pop = mutation.mutation(pop)
            evo_count += 1
        if verbose:
            print(f"--- {env_name} {algo}: global steps {total_steps}, steps {[a.steps[-1] for a in pop]}, regret "
                  f"{[round(float(r), 2) for r in regrets]}, fitness {[round(f, 2) for f in fitnesses]}, "
                  f"mean loss {[round(x[-1], 4) for x in pop_loss]}, agents {[a.index for a in pop]}, "
                  f"mutations {[a.mut for a in pop]}")
        if checkpoint is not None and pop[0].steps[-1] // checkpoint > checkpoint_count:
            for i, agent in enumerate(pop):  # save_population_checkpoint (utils.py:1126-1135)
                agent.save_checkpoint(f"{save_path}_{i}.pt" if overwrite_checkpoints
                                      else f"{save_path}_{i}_{agent.steps[-1]}.pt")
            checkpoint_count += 1
    return pop, pop_fitnesses

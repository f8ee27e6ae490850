"""Drop-in ``train_offline`` (agilerl/training/train_offline.py:30-364) for
CQN populations on the agx HBM replay buffer.

The dataset — any mapping with ``observations``, ``actions``, ``rewards`` and
``terminals`` (numpy arrays, or h5py-style datasets read with ``[...]``) — is
paired into transitions (row i with the observation of row i + 1, :177-201)
and written into the replay buffer in bulk, one ``memory.add`` per chunk
instead of one per row, leaving the ring exactly as the reference's
row-by-row fill leaves it.  The actions are checked once on the host to be
integers in [0, n): that is the loss kernel's precondition (agx_cqn.h).

A generation is ``evo_steps`` back-to-back updates per agent with no env step
in between (:242-254).  Each update samples through ``Sampler`` (the
reference's index stream) and runs ``agent.learn_device``: the loss stays on
the device, is added to a running sum there and read once per agent per
generation, so the updates — replayed from a captured graph from the second
one on (algorithms/learn_graph.py) — are enqueued without a host round trip.
Then every agent is evaluated with ``agent.test``; with a tournament AND a
mutation object (as the reference) the tournament replaces the population,
the elite is saved when ``save_elite``, and ``mutation.mutation`` mutates it;
a population checkpoint is written every ``checkpoint`` steps, to the file
names ``train_on_policy`` here uses.  Returns (pop, pop_fitnesses).

Single process only.  ``minari_dataset_id`` and ``swap_channels`` are outside
this path and raise; ``accelerator`` and ``wb`` are ignored, as by
``train_on_policy`` here.
"""

from __future__ import annotations

import warnings
from datetime import datetime

import numpy as np
import torch

from ..components.sampler import Sampler

_CHUNK = 1 << 16  # rows per memory.add


def dataset_transitions(dataset, n_actions: int) -> dict[str, np.ndarray]:
    """The dataset's len - 1 transitions as arrays with a leading row
    dimension (train_offline.py:177-201: row i's next_obs is observations[i + 1];
    done = bool(terminals[i])).  Raises ValueError unless every action is an
    integer in [0, n_actions)."""
    obs = np.asarray(dataset["observations"][...])
    actions = np.asarray(dataset["actions"][...])
    rewards = np.asarray(dataset["rewards"][...])
    terminals = np.asarray(dataset["terminals"][...])
    n = rewards.shape[0] - 1
    if n < 1:
        raise ValueError("the dataset needs at least two rows (row i is paired with the observation of row i + 1)")
    actions = actions[:n].reshape(n, -1)
    if actions.shape[1] != 1:
        raise ValueError(f"Discrete actions: expected one action per row, got shape {actions.shape[1:]}")
    whole = actions.astype(np.int64)
    if not (np.all(whole == actions) and whole.min() >= 0 and whole.max() < n_actions):
        raise ValueError(f"dataset actions must be integers in [0, {n_actions})")
    if obs.dtype.kind == "f":
        obs = obs.astype(np.float32, copy=False)
    return {"obs": obs[:n], "action": whole,
            "reward": rewards[:n].astype(np.float32).reshape(n, 1), "next_obs": obs[1:n + 1],
            "done": terminals[:n].astype(bool).astype(np.float32).reshape(n, 1)}


def fill_memory(memory, dataset, n_actions: int, chunk: int = _CHUNK) -> int:
    """Write the dataset's transitions into ``memory`` in chunks of at most
    ``min(chunk, memory.max_size)`` rows (a chunk wraps the ring at most
    once); -> the number of transitions."""
    rows = dataset_transitions(dataset, n_actions)
    n = rows["reward"].shape[0]
    step = max(1, min(int(chunk), int(memory.max_size)))
    for lo in range(0, n, step):
        memory.add({k: v[lo:lo + step] for k, v in rows.items()})
    return n


def train_offline(env, env_name: str, dataset, algo: str, pop, memory, INIT_HP=None, MUT_P=None,
                  swap_channels: bool = False, max_steps: int = 1_000_000, evo_steps: int = 10_000,
                  eval_steps=None, eval_loop: int = 1, target: float | None = None, tournament=None, mutation=None,
                  checkpoint=None, checkpoint_path=None, overwrite_checkpoints: bool = False,
                  save_elite: bool = False, elite_path=None, wb: bool = False, verbose: bool = True,
                  accelerator=None, minari_dataset_id=None, remote: bool = False, wandb_api_key=None):
    assert isinstance(algo, str), "'algo' must be the name of the algorithm as a string."
    assert isinstance(max_steps, int), "Number of steps must be an integer."
    assert isinstance(evo_steps, int), "Evolution frequency must be an integer."
    if target is not None:
        assert isinstance(target, (float, int)), "Target score must be a float or an integer."
    if checkpoint is not None:
        assert isinstance(checkpoint, int), "Checkpoint must be an integer."
    if save_elite is False and elite_path is not None:
        warnings.warn("'save_elite' set to False but 'elite_path' has been defined, elite will not "
                      "be saved unless 'save_elite' is set to True.", stacklevel=2)
    if checkpoint is None and checkpoint_path is not None:
        warnings.warn("'checkpoint' set to None but 'checkpoint_path' has been defined, checkpoint will not "
                      "be saved unless 'checkpoint' is defined.", stacklevel=2)
    if minari_dataset_id:
        raise NotImplementedError("minari datasets are outside the agx path: pass the dataset as a mapping of arrays")
    if swap_channels:
        raise NotImplementedError("swap_channels: store the dataset's frames channels-first")
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("train_offline runs in a single process (a sharded offline loop is out of scope)")
    save_path = (checkpoint_path.split(".pt")[0] if checkpoint_path is not None
                 else f"{env_name}-EvoHPO-{algo}-{datetime.now().strftime('%m%d%Y%H%M%S')}")

    fill_memory(memory, dataset, int(pop[0].action_dim))
    sampler = Sampler(memory=memory)
    pop_loss: list[list[float]] = [[] for _ in pop]
    pop_fitnesses: list[list[float]] = []
    total_steps = 0
    checkpoint_count = 0
    if mutation is not None:  # pre-training mutation (:233-235)
        pop = mutation.mutation(pop, pre_training_mut=True)

    while np.less([agent.steps[-1] for agent in pop], max_steps).all():
        for agent_idx, agent in enumerate(pop):
            total = torch.zeros((), dtype=torch.float64, device=agent.device)
            for _ in range(evo_steps):
                total += agent.learn_device(sampler.sample(agent.batch_size))
            pop_loss[agent_idx].append(float(total.item()) / max(evo_steps, 1))  # the generation's one read
            agent.steps[-1] += evo_steps
            total_steps += evo_steps
        fitnesses = [agent.test(env, swap_channels=swap_channels, max_steps=eval_steps, loop=eval_loop)
                     for agent in pop]
        pop_fitnesses.append(fitnesses)
        for agent in pop:
            agent.steps.append(agent.steps[-1])
        if target is not None and np.all(np.greater([np.mean(a.fitness[-10:]) for a in pop], target)) \
                and len(pop[0].steps) >= 100:
            return pop, pop_fitnesses
        if tournament and mutation is not None:  # tournament_selection_and_mutation (utils.py:1137-1225)
            elite, pop = tournament.select(pop)
            if save_elite and elite is not None:
                # the unmutated clone of the best agent (utils.py:1214-1223)
                elite_save_path = elite_path.split(".pt")[0] if elite_path is not None else f"{env_name}-elite_{algo}"
                elite.save_checkpoint(f"{elite_save_path}.pt")
            pop = mutation.mutation(pop)
        if verbose:
            print(f"--- {env_name} {algo}: global steps {total_steps}, steps {[a.steps[-1] for a in pop]}, fitness "
                  f"{[round(f, 2) for f in fitnesses]}, mean loss {[round(x[-1], 4) for x in pop_loss]}, "
                  f"agents {[a.index for a in pop]}, mutations {[a.mut for a in pop]}")
        if checkpoint is not None and pop[0].steps[-1] // checkpoint > checkpoint_count:
            for i, agent in enumerate(pop):  # save_population_checkpoint (utils.py:1126-1135)
                agent.save_checkpoint(f"{save_path}_{i}.pt" if overwrite_checkpoints
                                      else f"{save_path}_{i}_{agent.steps[-1]}.pt")
            checkpoint_count += 1
    return pop, pop_fitnesses

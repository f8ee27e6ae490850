"""Which [E, P, S] minibatch permutation the next PPO learn() gets, and where
numpy's global MT19937 stream has to stand afterwards.

Two layers: ``ShuffleStream`` is the bookkeeping of the global stream (numpy
only: it runs without a device), ``MinibatchOrders`` adds the transport to
the GPU (pinned staging, the side stream, the draw made ahead).  Both read
the population's values (P, S, update_epochs, perm_source, ...) when they
draw: mutations and tests change them after construction.

target_kl and the global numpy stream (ppo.py:836-842, 917-918)

The reference's agents learn one after another, each drawing one
np.random.shuffle per epoch it actually runs; an agent that stops early
on target_kl draws fewer.  The engine draws every agent's E shuffles
before the learn (all agents run at once), so after an early stop:
  * agents after the first early-stopping agent learn from shuffles
    that are shifted against the reference's (agent p's would start at
    shuffle sum(epochs_run[:p]), which is only known once every agent
    before it has finished — a serial dependency the population breaks);
  * the GLOBAL stream is put back in step: once the learn's epochs_run
    is known, the state is rewound to before the draw and advanced by
    exactly sum(epochs_run) shuffles, the reference's count, so every
    later consumer (tournament and mutation draws, the next learn) sees
    the state the reference would.
Without target_kl every agent runs all its epochs and both are exact.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from ..rng import numpy_shuffle_perms, numpy_shuffle_perms_shard


def draw_host_perms(out: np.ndarray, agent_epochs, heterogeneous: bool, global_P: int, agent_offset: int = 0,
                    global_epochs=None, scratch: dict | None = None) -> None:
    """[E, P, S] from the global numpy stream into ``out``: the shuffles of
    agents agent_offset .. agent_offset + P of ``global_P``, in the global
    agent order (rng.py).  An agent with fewer epochs than E draws fewer
    shuffles; its rows beyond get arange(S), so no row of the (reused,
    uninitialised pinned) buffer ever holds an out-of-range index — the
    gather prologue and the PyTorch learner index with every row."""
    E, P, S = out.shape
    if global_P == P:
        numpy_shuffle_perms(P, E, S, out=out, epochs_per_agent=agent_epochs if heterogeneous else None)
    else:
        eg = list(global_epochs)
        eg[agent_offset:agent_offset + P] = agent_epochs
        numpy_shuffle_perms_shard(out, agent_offset, global_P, eg, scratch)
    for p, e in enumerate(agent_epochs):
        if e < E:
            out[e:, p, :] = np.arange(S, dtype=np.int64)


def _ints(x) -> list[int]:
    return [int(v) for v in (x.tolist() if hasattr(x, "tolist") else x)]


class ShuffleStream:
    """The next learn's rows and the global stream's state, on the host."""

    def __init__(self, pop):
        self.pop = pop
        # numpy state before the current learn's shuffles, and the correction
        # a target-KL learn owes the global stream once its epochs_run is known
        self.drawn_state = None
        self.pending = None
        # a generation's shuffles drawn ahead by the population engine, agent by
        # agent (set_block): [K, E, P, S], learn k reads row k
        self.block = None
        self.k = 0
        self.ran: list = []
        self.scratch: dict = {}

    def set_block(self, block: np.ndarray | None) -> None:
        pop = self.pop
        if block is not None and (block.ndim != 4 or block.shape[1:] != (pop.update_epochs, pop.P, pop.S)):
            raise ValueError(f"generation shuffles {block.shape}, expected [K, {pop.update_epochs}, {pop.P}, "
                             f"{pop.S}]")
        self.block, self.k, self.ran = block, 0, []

    @property
    def exhausted(self) -> bool:
        """The generation's learns are all served."""
        return self.block is not None and self.k >= self.block.shape[0]

    def take_row(self) -> int:
        """Index of the next learn's row of the generation block."""
        if self.k >= self.block.shape[0]:
            raise RuntimeError("more learns than the generation's shuffles were drawn for")
        self.k += 1
        return self.k - 1

    def give_back_row(self) -> None:
        self.k -= 1  # served again by the next take

    def fill(self, out: np.ndarray):
        """The next learn's [E, P, S] permutations into ``out``; -> the global
        numpy state before the draw (None when they come from the engine's
        generation block, which owns the stream)."""
        if self.block is not None:
            np.copyto(out, self.block[self.take_row()])
            return None
        self.settle()
        pop = self.pop
        state = np.random.get_state(legacy=True)
        draw_host_perms(out, pop.agent_epochs, pop.heterogeneous, pop.global_P, pop.agent_offset,
                        pop.global_epochs, self.scratch)
        return state

    @staticmethod
    def rewind(state) -> None:
        np.random.set_state(state)  # undo a draw made ahead

    def report(self, epochs_run) -> None:
        """A learn has been enqueued whose agents ran ``epochs_run`` epochs."""
        pop = self.pop
        if pop.target_kl is None:
            return
        if self.block is not None:
            self.ran.append(self._keep(epochs_run))  # the engine re-syncs the stream
            return
        if pop.perm_source != "numpy" or self.drawn_state is None:
            return
        planned = list(pop.agent_epochs) if pop.heterogeneous else [pop.update_epochs] * pop.P
        self.pending = (self.drawn_state, planned, epochs_run, self._ready_mark())
        self.drawn_state = None

    def _keep(self, epochs_run):
        return epochs_run

    def _ready_mark(self):
        return None

    def settle(self) -> None:
        """Apply the correction a target-KL learn owes the global numpy stream
        (waits for that learn's epochs_run; see the module docstring).  Called
        before anything draws from the stream: the next permutation draw,
        tournament and mutation draws (discard)."""
        if self.pending is None:
            return
        state, planned, epochs_run, ready = self.pending
        self.pending = None
        if ready is not None:
            ready.synchronize()
        ran = _ints(epochs_run)
        if ran == planned:
            return
        np.random.set_state(state)
        if sum(ran):
            numpy_shuffle_perms(1, sum(ran), self.pop.S)

    def generation_epochs_run(self) -> list[list[int]]:
        """epochs_run of every target-KL learn served from the current block."""
        return [_ints(t) for t in self.ran]


class Ahead(NamedTuple):
    """The draw made ahead for the next learn."""
    perms: torch.Tensor
    event: "torch.cuda.Event | None"
    numpy_state: tuple | None
    from_block: bool


class MinibatchOrders(ShuffleStream):
    """[E, P, S] int64 device permutations, learn after learn."""

    def __init__(self, pop):
        super().__init__(pop)
        self.ahead: Ahead | None = None
        self._side = None
        self._host = None  # two pinned [E, P, S] buffers, each with the event of the copy that last read it
        self._turn = 0
        self._block_d = None

    def _keep(self, epochs_run):
        return torch.as_tensor(epochs_run).detach().clone()  # the learner reuses its buffer

    def _ready_mark(self):
        if self.pop.device.type != "cuda":
            return None
        ev = torch.cuda.Event()
        ev.record()
        return ev

    # -- the three sources, each used by permutations() and prefetch()
    def _from_block(self) -> bool:  # the generation block in HBM serves the rows
        return self.pop.perm_source == "numpy" and self._block_d is not None

    def _host_draw(self, side):
        """Host shuffle into pinned staging and its H2D copy on ``side``
        (None: the current stream); -> perms, the copy's event, numpy state."""
        host = self._host_buffer()
        state = self.fill(host.numpy())
        with torch.cuda.stream(side):
            perms = host.to(self.pop.device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self._host[self._turn ^ 1][1] = ev
        return perms, ev, state

    def _device_draw(self) -> torch.Tensor:
        pop = self.pop
        keys = torch.rand(pop.update_epochs, pop.P, pop.S, generator=pop.gen, device=pop.device)
        return torch.argsort(keys, dim=-1)

    def _host_buffer(self) -> torch.Tensor:
        """One of two pinned [E, P, S] int64 host buffers, alternating (the H2D
        copy that last read a buffer finished long before it is reused: it
        precedes a whole learn() on the stream; checked by its event)."""
        self.alloc_staging()
        slot = self._host[self._turn]
        self._turn ^= 1
        if slot[1] is not None:
            slot[1].synchronize()
        return slot[0]

    def alloc_staging(self) -> None:
        pop = self.pop
        if self._host is None and pop.perm_source == "numpy":
            shape = (pop.update_epochs, pop.P, pop.S)
            self._host = [[torch.empty(shape, dtype=torch.int64, pin_memory=True), None] for _ in range(2)]

    # -- what PPOPopulation delegates to
    def permutations(self) -> torch.Tensor:
        """[E, P, S] int64 per-agent minibatch orders for the next learn():
        numpy's global np.random.shuffle stream (default, ppo.py:836-842) or a
        device draw.  Returns the draw made ahead by prefetch() if there is
        one (the same draw, in the same order, as drawing here)."""
        a = self.ahead
        if a is not None:
            self.ahead = None
            self.drawn_state = a.numpy_state
            main = torch.cuda.current_stream()
            if a.event is not None:
                main.wait_event(a.event)
            a.perms.record_stream(main)  # (a block row: the block stays allocated until this stream is past it)
            return a.perms
        if self._from_block():
            perms = self._block_d[self.take_row()]
            perms.record_stream(torch.cuda.current_stream(self.pop.device))
            return perms
        if self.pop.perm_source == "numpy":
            perms, _, self.drawn_state = self._host_draw(None)
            return perms
        return self._device_draw()

    def prefetch(self) -> None:
        """Draw the next learn's permutations now, off the critical path:
        device mode enqueues rand + a radix sort on a side stream (beside the
        learner and the next rollout); numpy mode runs the native host shuffle
        (~0.5 ms of host time while the GPU learns) and an async H2D copy.
        Anything else that draws from the global numpy generator in between
        (tournament selection, mutations) must call discard() first, so the
        draws stay in the reference's order."""
        pop = self.pop
        if self.ahead is not None or pop.device.type != "cuda" or self.exhausted:
            return  # (exhausted: the next block is drawn with the next generation)
        if self._side is None:
            self._side = torch.cuda.Stream(device=pop.device)
        side = self._side
        if self._from_block():
            self.ahead = Ahead(self._block_d[self.take_row()], None, None, True)
        elif pop.perm_source == "numpy":
            # waits for a target-KL learn's epochs_run (before any rollout launch)
            self.ahead = Ahead(*self._host_draw(side), False)
        else:
            side.wait_stream(torch.cuda.current_stream(pop.device))
            with torch.cuda.stream(side):
                perms = self._device_draw()
                ev = torch.cuda.Event()
                ev.record(side)
            self.ahead = Ahead(perms, ev, None, False)

    def discard(self) -> None:
        """Undo a draw made ahead: the global numpy state goes back to before
        it (a block row is served again), so the next consumer of the stream
        draws what it would have drawn without the prefetch (the permutations
        are re-drawn later)."""
        a = self.ahead
        if a is not None and a.from_block:
            self.ahead = None
            self.give_back_row()
        elif a is None or a.numpy_state is None:
            self.settle()  # nothing drawn ahead from numpy (device draws use the pop's own generator)
        else:
            self.ahead = None
            self.rewind(a.numpy_state)

    def set_generation_perms(self, block: np.ndarray | None) -> None:
        """The population engine's draw of this population's shuffles for a
        whole generation ([K, E, P, S] int64: learn k of local agent p visits
        block[k, e, p] in epoch e), drawn agent by agent over the global
        population as the reference's agents learn one after another
        (train_on_policy.py:210-248 -> ppo.py:836-842).  None: draw per learn."""
        self.discard()
        self.set_block(block)
        # the whole block in HBM once (one copy at the generation's start, before
        # any launch): each learn then takes its row without host work
        self._block_d = (torch.from_numpy(block).to(self.pop.device)
                         if block is not None and self.pop.device.type == "cuda" else None)

    def epochs_changed(self) -> None:
        """update_epochs changed: the staging buffers and any draw made ahead
        have the old E."""
        self._host = None
        self.discard()
        self.ahead = None

"""Drop-in RolloutBuffer with the (capacity, num_envs) SoA resident in HBM.

Constructor, ``add`` / ``compute_returns_and_advantages`` /
``get_tensor_batch`` / ``get`` / ``reset`` / ``size`` follow
agilerl/components/rollout_buffer.py (:61-582) for flat (non-recurrent)
Box / Discrete spaces.  ``compute_returns_and_advantages`` is one agx_gae
launch, bit-identical to the reference's NumPy loop (f64 carry, NumPy-2
dtype flow) for f32 ``last_value``.  Fields are plain tensors in a dict
(``tensordict`` is not a dependency); ``get_tensor_batch`` returns a dict.

``recurrent=True`` stores the hidden state each step was taken from, one HBM
tensor [capacity, num_envs, layers, hidden] per key, and serves truncated
BPTT (:676-922) from the device: ``prepare_sequence_tensors`` is one
agx_bptt_plan call (the sequence table; S, L and the sequences' lengths are
read back once), ``get_minibatch_sequences`` one agx_bptt_gather launch per
minibatch (include/agx_bptt.h).  Vector Box observations only.
"""

from __future__ import annotations

import warnings

import numpy as np
import torch

from .. import kernels as K


def _obs_shape(space) -> tuple[int, ...]:
    if hasattr(space, "n") and not getattr(space, "shape", None):
        return (1,)
    return tuple(space.shape)


def _num_actions(space) -> int:
    if hasattr(space, "n") and not getattr(space, "shape", None):  # Discrete
        return 1
    return int(np.prod(space.shape))


class RolloutBuffer:
    def __init__(self, capacity: int, observation_space, action_space, num_envs: int = 1, device="cuda",
                 gae_lambda: float = 0.95, gamma: float = 0.99, recurrent: bool = False,
                 hidden_state_architecture=None, use_gae: bool = True, wrap_at_capacity: bool = False,
                 max_seq_len: int | None = None, bptt_sequence_type=None) -> None:
        if recurrent and hidden_state_architecture is None:
            raise ValueError("hidden_state_architecture must be provided if recurrent=True")
        if recurrent and len(_obs_shape(observation_space)) != 1:
            raise NotImplementedError("recurrent agx rollout storage takes vector Box observations")
        self.capacity = int(capacity)
        self.observation_space = observation_space
        self.action_space = action_space
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.gamma = float(gamma)
        self.gae_lambda = float(gae_lambda)
        self.recurrent = recurrent
        self.hidden_state_architecture = hidden_state_architecture
        self.use_gae = use_gae
        self.wrap_at_capacity = wrap_at_capacity
        self.max_seq_len = max_seq_len
        self.bptt_sequence_type = bptt_sequence_type
        self.pos = 0
        self.full = False
        self.num_sequences = self.max_sequence_length = None
        self._plan = self._unpadded_slices = None
        self._initialize_buffers()

    def _initialize_buffers(self) -> None:
        C, N, dev = self.capacity, self.num_envs, self.device
        obs = _obs_shape(self.observation_space)
        f32 = dict(dtype=torch.float32, device=dev)
        self.buffer = {
            "observations": torch.zeros((C, N, *obs), **f32),
            "next_observations": torch.zeros((C, N, *obs), **f32),
            "actions": torch.zeros((C, N, _num_actions(self.action_space)), **f32),
            "rewards": torch.zeros((C, N), **f32),
            "dones": torch.zeros((C, N), dtype=torch.bool, device=dev),
            "values": torch.zeros((C, N), **f32),
            "log_probs": torch.zeros((C, N), **f32),
            "advantages": torch.zeros((C, N), **f32),
            "returns": torch.zeros((C, N), **f32),
            "episode_starts": torch.zeros((C, N), dtype=torch.bool, device=dev),
        }
        if self.recurrent:
            # {key: (layers, num_envs, hidden)} -> [capacity, num_envs, layers, hidden] per key (:203-223)
            self.buffer["hidden_states"] = {k: torch.zeros((C, N, int(sh[0]), int(sh[2])), **f32)
                                            for k, sh in self.hidden_state_architecture.items()}
        self._gae_ws = None

    # ------------------------------------------------------------------ #
    def size(self) -> int:
        return (self.capacity if self.full else self.pos) * self.num_envs

    def reset(self) -> None:
        self.pos = 0
        self.full = False

    def _put(self, key: str, value, shape, dtype=None) -> None:
        t = torch.as_tensor(value, dtype=dtype) if not isinstance(value, torch.Tensor) else value
        self.buffer[key][self.pos].copy_(t.reshape(shape), non_blocking=True)

    def add(self, obs, action, reward, done, value, log_prob, next_obs=None, hidden_state=None,
            next_hidden_state=None, episode_start=None, action_mask=None) -> None:
        if self.pos == self.capacity:
            if not self.wrap_at_capacity:
                raise ValueError(f"Buffer has reached capacity ({self.capacity} transitions) but received more "
                                 "transitions. Either increase capacity or set wrap_at_capacity=True.")
            self.pos = 0
        N = self.num_envs
        obs_shape = self.buffer["observations"].shape[2:]
        self._put("observations", obs, (N, *obs_shape), torch.float32)
        self._put("actions", action, (N, -1))
        self._put("rewards", reward, (N,), torch.float32)
        self._put("dones", done, (N,), torch.bool)
        self._put("values", value, (N,), torch.float32)
        self._put("log_probs", log_prob, (N,), torch.float32)
        if next_obs is not None:
            self._put("next_observations", next_obs, (N, *obs_shape), torch.float32)
        if episode_start is not None:
            self._put("episode_starts", episode_start, (N,), torch.bool)
        else:
            self.buffer["episode_starts"][self.pos].zero_()
        if action_mask is not None:
            m = torch.as_tensor(action_mask, dtype=torch.bool).reshape(N, -1)
            if "action_masks" not in self.buffer:
                self.buffer["action_masks"] = torch.ones((self.capacity, N, m.shape[-1]), dtype=torch.bool,
                                                         device=self.device)
            self.buffer["action_masks"][self.pos].copy_(m)
        if self.recurrent and hidden_state is not None:  # (layers, num_envs, hidden) -> (num_envs, layers, hidden)
            for k, h in hidden_state.items():
                self.buffer["hidden_states"][k][self.pos].copy_(torch.as_tensor(h).permute(1, 0, 2))
        self._plan = self._unpadded_slices = None
        self.pos += 1
        if self.pos == self.capacity:
            self.full = True

    def fused_step(self, agent, obs, action_mask, hidden_state, reset=None):
        """One fused recurrent policy step (``agent.fused_policy_step``) that writes slot ``pos`` itself: the
        observation, action, log-prob, value and the hidden state the step was taken from (zeros for the rows
        flagged in ``reset``).  -> (action, log_prob, value as host arrays, next hidden state), with
        ``finish_step`` to follow, or None where the kernel does not apply (nothing is written)."""
        if self.pos == self.capacity:
            if not self.wrap_at_capacity:
                raise ValueError(f"Buffer has reached capacity ({self.capacity} transitions) but received more "
                                 "transitions. Either increase capacity or set wrap_at_capacity=True.")
            self.pos = 0
        b, p, N = self.buffer, self.pos, self.num_envs
        out = {k: b[k][p] for k in ("actions", "log_probs", "values")}
        res = agent.fused_policy_step(agent.preprocess_observation(obs), action_mask, hidden_state, reset=reset,
                                      out=out, store_hidden={k: v[p] for k, v in b["hidden_states"].items()},
                                      store_obs=b["observations"][p])
        if res is None:
            return None
        host = torch.cat([out["actions"].reshape(-1), out["log_probs"], out["values"]]).cpu().numpy()
        return agent.host_action(host[:-2 * N].reshape(N, -1)), host[-2 * N:-N], host[-N:], res["hidden"]

    def finish_step(self, reward, done, next_obs=None, action_mask=None) -> None:
        """The host's half of a slot ``fused_step`` wrote: what the env returned, then the slot is taken."""
        N = self.num_envs
        self._put("rewards", reward, (N,), torch.float32)
        self._put("dones", done, (N,), torch.bool)
        if next_obs is not None:
            self._put("next_observations", next_obs, (N, *self.buffer["observations"].shape[2:]), torch.float32)
        self.buffer["episode_starts"][self.pos].zero_()
        if action_mask is not None:
            m = torch.as_tensor(action_mask, dtype=torch.bool).reshape(N, -1)
            if "action_masks" not in self.buffer:
                self.buffer["action_masks"] = torch.ones((self.capacity, N, m.shape[-1]), dtype=torch.bool,
                                                         device=self.device)
            self.buffer["action_masks"][self.pos].copy_(m)
        self._plan = self._unpadded_slices = None
        self.pos += 1
        if self.pos == self.capacity:
            self.full = True

    # ------------------------------------------------------------------ #
    def compute_returns_and_advantages(self, last_value, last_done) -> None:
        """GAE (or Monte-Carlo returns) over the filled prefix, rollout_buffer.py:413-481."""
        T = self.capacity if self.full else self.pos
        if T == 0:
            return
        N, dev = self.num_envs, self.device
        lv = torch.as_tensor(last_value).to(dev, torch.float32).reshape(1, N).contiguous()
        ld = torch.as_tensor(last_done).to(dev).reshape(1, N).to(torch.uint8).contiguous()
        b = self.buffer
        rew = b["rewards"][:T].reshape(1, T, N)
        done = b["dones"][:T].view(torch.uint8).reshape(1, T, N)
        val = b["values"][:T].reshape(1, T, N)
        out = K.gae(rew, done, val, lv, ld, self.gamma, self.gae_lambda, self.use_gae,
                    advantages=b["advantages"][:T].reshape(1, T, N), returns=b["returns"][:T].reshape(1, T, N),
                    with_stats=self.recurrent)
        # recurrent: the launch's mean / unbiased std of the advantages, for normalize_advantages
        self._adv_stats = (T, out[2]) if self.recurrent else None

    def normalize_advantages(self) -> None:
        """(a - mean) / (std + 1e-8) over the filled prefix in place (ppo.py:935-944), from the statistics the
        GAE launch took: one agx_adv_normalize launch.  Applies once per compute_returns_and_advantages."""
        stats = getattr(self, "_adv_stats", None)
        if stats is None:
            raise ValueError("normalize_advantages() follows compute_returns_and_advantages() on a recurrent buffer")
        T, st = stats
        K.adv_normalize_(self.buffer["advantages"][:T], st)
        self._adv_stats = None

    def _flat_items(self):
        """The per-step tensors (the nested hidden states are served by get_minibatch_sequences)."""
        return [(k, v) for k, v in self.buffer.items() if k != "hidden_states"]

    def get_tensor_batch(self, batch_size: int | None = None, device=None) -> dict[str, torch.Tensor]:
        target = torch.device(device) if device is not None else self.device
        T = self.capacity if self.full else self.pos
        total = T * self.num_envs
        if total == 0:
            return {}
        flat = {k: v[:T].reshape(total, *v.shape[2:]) for k, v in self._flat_items()}
        if batch_size is not None:
            if batch_size > total:
                warnings.warn(f"Batch size {batch_size} is larger than buffer_size {total}. Returning all data.",
                              stacklevel=2)
            else:
                idx = torch.randperm(total, device="cpu")[:batch_size].to(self.device)
                flat = {k: v.index_select(0, idx) for k, v in flat.items()}
        return {k: v.to(target) for k, v in flat.items()}

    def get(self, batch_size: int | None = None) -> dict[str, np.ndarray]:
        T = self.capacity if self.full else self.pos
        total = T * self.num_envs
        if total == 0:
            return {}
        flat = {k: v[:T].reshape(total, *v.shape[2:]) for k, v in self._flat_items()}
        if batch_size is not None and batch_size <= total:
            idx = torch.as_tensor(np.random.choice(total, size=batch_size, replace=False)).to(self.device)
            flat = {k: v.index_select(0, idx) for k, v in flat.items()}
        elif batch_size is not None:
            warnings.warn(f"Batch size {batch_size} is larger than buffer size {total}. Returning all data.",
                          stacklevel=2)
        return {k: v.cpu().numpy() for k, v in flat.items()}

    # ---- truncated BPTT (rollout_buffer.py:676-922) ---------------------------
    def prepare_sequence_tensors(self, device=None) -> None:
        """The sequence table of the filled prefix: ``num_sequences``, ``max_sequence_length`` (the longest
        sequence, as the reference pads to) and ``unpadded_slices``; the padded tensors themselves are built
        per minibatch.  The caller normalises the advantages first (ppo.py:935-944)."""
        if not self.recurrent:
            raise ValueError("prepare_sequence_tensors() is only supported when recurrent=True.")
        if self.size() == 0:
            raise ValueError("Attempting to prepare sequences with empty buffer.")
        T = self.capacity if self.full else self.pos
        seq, row_offset, meta = K.bptt_plan(self.buffer["dones"][:T], self.max_seq_len, self.bptt_sequence_type)
        S, L, _rows, _ = (int(x) for x in meta.cpu())  # the one read-back of a learn()
        self.num_sequences, self.max_sequence_length = S, L
        self._plan = (T, seq, row_offset, seq[:S, 2].cpu().to(torch.int64))
        self._unpadded_slices = None

    @property
    def unpadded_slices(self):
        """The flat step indices t * num_envs + env of every sequence (:765-775), built on first use."""
        if self._plan is None:
            return None
        if self._unpadded_slices is None:
            N = self.num_envs
            self._unpadded_slices = [torch.arange(n) * N + (s * N + e)
                                     for e, s, n in self._plan[1][:self.num_sequences].cpu().tolist()]
        return self._unpadded_slices

    def get_minibatch_sequences(self, batch_size: int):
        """Yields (padded, unpadded) dicts of minibatches of whole sequences (:845-922): padded holds
        observations / actions / pad_mask (/ action_masks) over [sequences * max_sequence_length] rows and
        initial_hidden_states {key: [layers, sequences, hidden]} (already in the LSTM's order); unpadded holds
        log_probs / advantages / values / returns of the valid rows, and their padded rows as valid_row."""
        if self._plan is None:
            raise ValueError("Attempting to fetch minibatches before preparing sequences. "
                             "Call prepare_sequence_tensors() first.")
        S, L = self.num_sequences, self.max_sequence_length
        if batch_size > S:
            warnings.warn(f"Batch size {batch_size} is larger than the number of sequences ({S}), using "
                          f"batch_size = {S}.", stacklevel=2)
            batch_size = S
        T, seq, _row_offset, lens = self._plan
        order = torch.randperm(S)  # the CPU generator, as the reference draws it
        ids_dev = order.to(self.device)
        b = self.buffer
        for start in range(0, S, batch_size):
            ids = order[start:start + batch_size]
            n = lens[ids]
            local = (torch.cumsum(n, 0) - n).to(torch.int32).to(self.device)
            out = K.bptt_gather(seq, S, ids_dev[start:start + batch_size], local, int(n.sum()), L,
                                b["observations"][:T], b["actions"][:T], b["log_probs"][:T], b["advantages"][:T],
                                b["returns"][:T], b["values"][:T],
                                mask=b["action_masks"][:T] if "action_masks" in b else None,
                                hidden={k: v[:T] for k, v in b["hidden_states"].items()})
            unpadded = {k: out.pop(k) for k in ("log_probs", "advantages", "values", "returns", "valid_row")}
            yield out, unpadded

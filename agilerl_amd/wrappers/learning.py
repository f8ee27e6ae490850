"""``BanditEnv`` (agilerl/wrappers/learning.py:40-92): a labelled dataset as
a contextual-bandit environment.  ``reset() -> context``, ``step(arm) ->
(context, reward)``; a context is ``[arms, arms * features]``, row k holding
the drawn feature row in block k and zeros elsewhere; the reward is 1 for
the drawn row's class, read from the context the arm was chosen in.  Rows are
drawn with Python's ``random``, as the reference draws them.

``features`` / ``targets``: pandas DataFrames (rows read by label with
``.loc``, as the reference) or numpy arrays; pandas is imported only when a
DataFrame is passed in."""

from __future__ import annotations

import random

import numpy as np


def _factorize(values: np.ndarray) -> np.ndarray:
    """pd.factorize's codes: classes numbered in order of first appearance."""
    codes: dict = {}
    return np.array([codes.setdefault(v.item() if hasattr(v, "item") else v, len(codes)) for v in values],
                    dtype=np.int64)


class BanditEnv:
    def __init__(self, features, targets) -> None:
        frame = hasattr(features, "loc")
        t = np.asarray(targets.values if hasattr(targets, "values") else targets)
        first = t.reshape(len(t), -1)[:, 0]  # targets.nunique()[0]: the first column's classes
        self.arms = int(len({v.item() if hasattr(v, "item") else v for v in first if v == v}))
        row0 = np.array(features.loc[0]) if frame else np.asarray(features)[0]
        self.context_dim = (len(row0) * self.arms,)
        self.features = features
        self._row = (lambda r: np.array(features.loc[r])) if frame else (lambda r: np.array(np.asarray(features)[r]))
        self.targets = _factorize(t.ravel())
        self.prev_reward = np.zeros(self.arms)

    def _new_state_and_target_action(self):
        r = random.randint(0, len(self.features) - 1)
        context = self._row(r)
        target = self.targets[r]
        next_state = np.zeros((self.arms, *self.context_dim))
        for i, j in zip(range(self.arms), range(0, self.context_dim[0], len(context))):
            next_state[i, j:j + len(context)] = context
        return next_state, target

    def step(self, k: int):
        reward = self.prev_reward[k]
        next_state, target = self._new_state_and_target_action()
        next_reward = np.zeros(self.arms)
        next_reward[target] = 1
        self.prev_reward = next_reward
        return next_state, reward

    def reset(self):
        next_state, target = self._new_state_and_target_action()
        next_reward = np.zeros(self.arms)
        next_reward[target] = 1
        self.prev_reward = next_reward
        return next_state

"""GPU UserCF similarity: drop-in for src/similarity/user_cf.py:11-94.

The reference ships this calculator but comments it out of its pipeline
(recall_pipeline.py:137,151-155): its Python loop is O(sum_items n_i^2) and
keeps every user pair in a dict.  ``compute()`` produces each user's top
``usercf_sim_user_topk`` neighbours on the device (nrk_usercf_topn,
csrc/usercf.hip) without materialising the u2u matrix, which is all
UserCFRecaller reads.  ``calculate()`` / ``UserCFResult.to_dict()`` return
the reference's ``{user_i: {user_j: sim}}`` -- same row order, same entry
order, bit-identical fp64 values -- for logs small enough to hold it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from .. import ops
from ..config import RecallConfig
from ..data.extractors import item_user_time_csr
from .base import BaseSimilarityCalculator


class UserCFResult:
    """Device top-n neighbours over dense user rows + the raw-id maps."""

    def __init__(self, inputs, user_ids, row_order, topn, cols, vals, cnt, nnz):
        self._inputs = inputs          # the six device arrays of ops.usercf_topn
        self.user_ids = user_ids       # dense -> raw (ascending)
        self.row_order = row_order     # dense rows in the reference's row (first encounter) order
        self._top = {int(topn): (cols, vals)}
        self.cnt, self.nnz = cnt, nnz  # click rows / distinct neighbours per dense row

    def top(self, topn: int):
        """(cols [U, topn] int32 dense rows -1 padded, vals [U, topn] f64)."""
        topn = int(topn)
        if topn not in self._top:
            oc, ov, _, _ = ops.usercf_topn(*self._inputs, topn=topn)
            self._top[topn] = (oc, ov)
        return self._top[topn]

    def to_dict(self) -> Dict[int, Dict[int, float]]:
        total = int(self.nnz.to(torch.int64).sum())
        if total >= 2**31:
            raise ValueError(f"the u2u matrix has {total} entries (>= 2^31): use compute(), whose top-n per user "
                             "never materialises it")
        row_off, v, s, f = ops.usercf_sim(*self._inputs, self.nnz)
        row_off, v, s, f = (x.cpu().numpy() for x in (row_off, v, s, f))
        rows = np.repeat(np.arange(len(self.user_ids)), np.diff(row_off))
        order = np.lexsort((f, rows))  # inside a row: first-encounter order
        ids = self.user_ids
        rv, rs = ids[v[order]].tolist(), s[order].tolist()
        out: Dict[int, Dict[int, float]] = {}
        for r in self.row_order.tolist():
            a, b = int(row_off[r]), int(row_off[r + 1])
            out[int(ids[r])] = dict(zip(rv[a:b], rs[a:b]))
        return out


class UserCFSimilarity(BaseSimilarityCalculator):
    def __init__(self, config: RecallConfig = None, device="cuda"):
        super().__init__(config or RecallConfig())
        self.device = torch.device(device)

    def compute(self, click_df, user_activate_degree_dict: Dict[int, float]) -> UserCFResult:
        items, i_off, users_raw, _ = item_user_time_csr(click_df)
        user_ids, i_users = np.unique(users_raw, return_inverse=True)
        n_items, n_users = len(items), len(user_ids)
        n_i = np.diff(i_off)
        item_of = np.repeat(np.arange(n_items), n_i)
        # every user's clicks sorted by item (the entries already are, so a stable sort by user)
        by_user = np.argsort(i_users, kind="stable")
        u_items = item_of[by_user]
        u_off = np.zeros(n_users + 1, np.int64)
        u_off[1:] = np.cumsum(np.bincount(i_users, minlength=n_users))
        # user_activate_degree_dict[u] (user_cf.py:51-53): a missing user is the reference's KeyError
        act = np.fromiter((float(user_activate_degree_dict[u]) for u in user_ids.tolist()), np.float64, n_users)
        # 1.0 / log_penalty(len(list)) with the host's math.log, once per distinct length
        lens, inv = np.unique(n_i, return_inverse=True)
        pen = np.array([1.0 / math.log(int(n) + 1) for n in lens], np.float64)[inv] if n_items else np.zeros(0)
        # row order: u2u_sim.setdefault(u, {}) at u's first entry of the item walk (user_cf.py:43)
        _, first_pos = np.unique(i_users, return_index=True)
        row_order = np.argsort(first_pos, kind="stable")
        d = self.device
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(d)  # noqa: E731
        inputs = (t(i_off, np.int64), t(i_users, np.int32), t(u_off, np.int64), t(u_items, np.int32),
                  t(act, np.float64), t(pen, np.float64))
        topn = self.config.usercf_sim_user_topk
        cols, vals, cnt, nnz = ops.usercf_topn(*inputs, topn=topn)
        return UserCFResult(inputs, user_ids.astype(np.int64), row_order, topn, cols, vals, cnt, nnz)

    def calculate(self, click_df, user_activate_degree_dict: Dict[int, float]) -> Dict:
        self.result = self.compute(click_df, user_activate_degree_dict)
        self.similarity_matrix = self.result.to_dict()
        return self.similarity_matrix

    def get_similar_users(self, user_id: int, topk: int = 20) -> List[Tuple[int, float]]:
        """user_cf.py:71-94."""
        if not self.is_calculated():
            raise ValueError("Similarity matrix not calculated. Call calculate() first.")
        if user_id not in self.similarity_matrix:
            return []
        return sorted(self.similarity_matrix[user_id].items(), key=lambda x: x[1], reverse=True)[:topk]

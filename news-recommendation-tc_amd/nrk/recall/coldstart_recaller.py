"""Cold-start recaller: drop-in for src/recall/coldstart_recaller.py:12-171.

The reference filters the lists of a base recall with four rules in a Python
loop over every (user, candidate) pair (:54-126) and sorts a user's survivors
on every ``recall`` (:128-147).  Here the constructor factorises the ids and
categories on the host (``dense_inputs``: pandas hash lookups, so Python's
``in`` / ``==`` semantics hold), puts the lists, one profile row per user and
four item tables on the device, and runs nrk_coldstart_filter once over every
pair; ``batch_recall`` is one nrk_coldstart_recall call for the whole batch.
``filtered_results`` and every returned list hold the base lists' own tuples,
taken by position: an int score stays an int, an item id of any hashable
type comes back as given.  There is no CPU fallback.
"""
from __future__ import annotations

from itertools import chain
from typing import Dict, List, Tuple

import numpy as np
import pandas as pd
import torch

from .. import ops
from .base import BaseRecaller

_EXACT = float(2**53)  # ints below it convert to f64 exactly, as Python's int - float does


def _obj(seq):
    """1-D object array, element by element (tuple ids stay tuples)."""
    return np.fromiter(seq, dtype=object, count=len(seq))


def _f64(values, what):
    """Python numbers -> f64, refusing an int that the conversion would round."""
    a = np.asarray(values)
    if a.dtype == object or (a.dtype.kind in "iu" and len(a) and float(np.abs(a).max()) >= _EXACT):
        raise ValueError(f"{what} must be numbers with |x| < 2^53")
    return a.astype(np.float64).reshape(-1)


def dense_inputs(base_recall_results, user_hist_item_types_dict, user_hist_item_words_dict,
                 user_last_item_created_time_dict, item_type_dict, item_words_dict, item_created_time_dict,
                 click_article_ids_set):
    """The reference's dicts as the dense arrays of nrk_coldstart_filter /
    nrk_coldstart_recall (include/nrk.h), on the host.  Returns (users, score
    [N] f64, tables): ``users`` are the lists' owners in dict order and
    ``tables`` is (list_off, item, prof, cat_off, cat, mean_words,
    last_created, item_type, item_words, item_created, item_clicked), the
    argument order of ops.coldstart_filter."""
    users = list(base_recall_results.keys())
    lists = [base_recall_results[u] for u in users]
    lens = np.fromiter((len(x) for x in lists), np.int64, count=len(lists))
    list_off = np.zeros(len(users) + 1, np.int64)
    list_off[1:] = np.cumsum(lens)
    flat = list(chain.from_iterable(lists))
    score = _f64([t[1] for t in flat], "scores") if flat else np.zeros(0)
    if np.isnan(score).any():
        raise ValueError("scores must not hold NaN")

    # item tables: one row per key of item_type_dict; a row missing from the
    # words or the created-time dict is never referenced (:86-91)
    keys = list(item_type_dict.keys())
    n_items = len(keys)
    full = np.fromiter((k in item_words_dict and k in item_created_time_dict for k in keys), bool, count=n_items)
    item = np.full(len(flat), -1, np.int32)
    clicked = np.zeros(n_items, np.uint8)
    if n_items:
        idx = pd.Index(_obj(keys), dtype=object, tupleize_cols=False)
        if flat:
            rows = idx.get_indexer(_obj([t[0] for t in flat]))
            item = np.where((rows >= 0) & full[np.maximum(rows, 0)], rows, -1).astype(np.int32)
        if len(click_article_ids_set):
            hit = idx.get_indexer(_obj(list(click_article_ids_set)))
            clicked[hit[hit >= 0]] = 1
    words = _f64([item_words_dict[k] if f else 0 for k, f in zip(keys, full)], "word counts")
    created = _f64([item_created_time_dict[k] if f else 0.0 for k, f in zip(keys, full)], "created times")

    # profile rows: the listed users that have a profile (:74); a profile
    # without a mean or a last-created time is the reference's KeyError (:81-82)
    known = [u for u in users if u in user_hist_item_types_dict]
    prow = {u: n for n, u in enumerate(known)}
    prof = np.fromiter((prow.get(u, -1) for u in users), np.int32, count=len(users))
    mean_words = _f64([user_hist_item_words_dict[u] for u in known], "mean word counts")
    last_created = _f64([user_last_item_created_time_dict[u] for u in known], "last created times")
    # categories of the items and of the users' sets, factorised together
    sets = [list(user_hist_item_types_dict[u]) for u in known]
    clens = np.fromiter((len(s) for s in sets), np.int64, count=len(sets))
    codes, _ = pd.factorize(_obj([item_type_dict[k] for k in keys] + list(chain.from_iterable(sets))),
                            use_na_sentinel=False)
    item_type, ucat = codes[:n_items].astype(np.int32), codes[n_items:].astype(np.int32)
    owner = np.repeat(np.arange(len(known)), clens)
    cat = ucat[np.lexsort((ucat, owner))]  # ascending inside every user
    cat_off = np.zeros(len(known) + 1, np.int64)
    cat_off[1:] = np.cumsum(clens)
    return users, score, (list_off, item, prof, cat_off, cat, mean_words, last_created, item_type, words, created,
                          clicked)


class ColdStartRecaller(BaseRecaller):
    def __init__(self, config, base_recall_results: Dict, user_hist_item_types_dict: Dict,
                 user_hist_item_words_dict: Dict, user_last_item_created_time_dict: Dict, item_type_dict: Dict,
                 item_words_dict: Dict, item_created_time_dict: Dict, click_article_ids_set, device="cuda"):
        super().__init__(config)
        self.base_recall_results = base_recall_results
        self.user_hist_item_types_dict = user_hist_item_types_dict
        self.user_hist_item_words_dict = user_hist_item_words_dict
        self.user_last_item_created_time_dict = user_last_item_created_time_dict
        self.item_type_dict = item_type_dict
        self.item_words_dict = item_words_dict
        self.item_created_time_dict = item_created_time_dict
        self.click_article_ids_set = click_article_ids_set
        self.device = torch.device(device)
        self.filtered_results = self._apply_filtering()

    def _apply_filtering(self) -> Dict:
        """coldstart_recaller.py:54-126 on the device."""
        users, score, tables = dense_inputs(
            self.base_recall_results, self.user_hist_item_types_dict, self.user_hist_item_words_dict,
            self.user_last_item_created_time_dict, self.item_type_dict, self.item_words_dict,
            self.item_created_time_dict, self.click_article_ids_set)
        self._list_of = {u: n for n, u in enumerate(users)}
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)  # noqa: E731
        self._score = d(score)
        self._tables = tuple(d(a) for a in tables)
        keep, kept = ops.coldstart_filter(*self._tables)
        keep, kept = keep.cpu().numpy(), kept.cpu().numpy()
        pos = (np.flatnonzero(keep) - np.repeat(tables[0][:-1], kept)).tolist()
        out = {}
        at = 0
        for n, u in enumerate(users):
            m = int(kept[n])
            if m:
                lst = self.base_recall_results[u]
                out[u] = [lst[p] for p in pos[at:at + m]]
                at += m
        return out

    def batch_recall(self, user_ids: List, topk: int = 10) -> Dict:
        """Every user of the batch in one nrk_coldstart_recall call."""
        user_ids = list(user_ids)
        if not user_ids:
            return {}
        t = self._tables
        q = torch.tensor([self._list_of.get(u, -1) for u in user_ids], dtype=torch.int64, device=self.device)
        opos, _, ocnt = ops.coldstart_recall(q, t[0], t[1], self._score, *t[2:], topk, validate=False)
        opos, ocnt = opos.cpu().numpy(), ocnt.cpu().numpy()
        out = {}
        for n, u in enumerate(user_ids):
            m = int(ocnt[n])
            lst = self.base_recall_results[u] if m else ()
            out[u] = [lst[p] for p in opos[n, :m].tolist()]
        return out

    def recall(self, user_id, topk: int = 10) -> List[Tuple]:
        """coldstart_recaller.py:128-147 on the GPU (a batch of one)."""
        return self.batch_recall([user_id], topk)[user_id]

    def get_statistics(self) -> Dict:
        """coldstart_recaller.py:149-171."""
        total_users = len(self.base_recall_results)
        cold_users = len(self.filtered_results)
        total_items = sum(len(x) for x in self.base_recall_results.values())
        cold_items = sum(len(x) for x in self.filtered_results.values())
        return {
            "total_users": total_users,
            "cold_start_users": cold_users,
            "cold_start_user_ratio": cold_users / total_users if total_users > 0 else 0,
            "total_items_before_filtering": total_items,
            "total_items_after_filtering": cold_items,
            "filtering_ratio": cold_items / total_items if total_items > 0 else 0,
        }

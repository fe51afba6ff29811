"""GPU RecallFusion: drop-in for src/recall/fusion.py.

Same plugin surface as the reference's ``RecallFusion`` (fusion.py:10-375):
``add_recall_result(name, result, weight)``, ``fuse(topk, user_history,
remove_seen)`` -> ``{user_id: [(item_id, score), ...]}``, ``save(path)`` (the
``all_recall_results.pkl`` wire format RecallPipeline writes,
recall_pipeline.py:276-294), the six fusion strategies and the three
normalisations.  Underneath, every user's merge runs on the GPU in one launch
(``nrk_fuse``, csrc/fusion.hip); the host side only flattens the result dicts
into arrays and builds the output dict.

Exactness: global / local min-max and every strategy run the reference's
float64 operations in the reference's order (bit-identical scores, identical
lists and tie order).  The z-score normalisation (:155-175) runs on the host
exactly as the reference does -- numpy mean / std of the method's scores and
numpy's exp for the sigmoid, so those scores are the reference's to the bit --
and the device takes them as pre-normalised.

``RecallEnsemble`` (fusion.py:419-556), the online counterpart over recaller
instances, feeds the same kernel: its merge is the local normalisation with
the first three strategies.
"""
from __future__ import annotations

import os
import pickle
from itertools import chain
from typing import Dict, List, Optional, Tuple

import numpy as np
import pandas as pd
import torch

from .. import ops
from .._lib import P, call

STRATEGIES = {"weighted_sum": 0, "weighted_avg": 1, "max_score": 2, "harmonic_mean": 3,
              "diversity_weighted": 4, "rrf": 5}
NORMS = {"local": 0, "global": 1, "z-score": 2}
FUSE_MAX = 256        # entries per user (and topk) of nrk_fuse (4 per lane, registers)
FUSE_WIDE_MAX = 2048  # entries per user of nrk_fuse_wide (LDS)


class RecallFusion:
    def __init__(self, config=None, fusion_strategy: str = "weighted_avg", normalize_method: str = "local",
                 device="cuda"):
        self.config = config
        self.recall_results: Dict[str, Dict] = {}
        self.weights: Dict[str, float] = {}
        self.fusion_strategy = fusion_strategy
        self.normalize_method = normalize_method
        self.device = torch.device(device)
        self.fused_results = None

    def add_recall_result(self, name: str, result: Dict[int, List[Tuple[int, float]]], weight: float = 1.0):
        """fusion.py:55-69."""
        self.recall_results[name] = result
        self.weights[name] = weight

    # ------------------------------------------------------------------ fuse --
    def fuse(self, topk: int = 30, user_history: Optional[Dict[int, set]] = None,
             remove_seen: bool = True) -> Dict[int, List[Tuple[int, float]]]:
        """fusion.py:267-342 on the device."""
        if not self.recall_results:
            raise ValueError("No recall results added. Use add_recall_result() first.")
        names = list(self.recall_results)
        # the reference's user order: a set updated method by method (:306-309)
        all_users = set()
        for nm in names:
            all_users.update(self.recall_results[nm].keys())
        users = list(all_users)
        if not users:
            self.fused_results = {}
            return {}
        uidx = pd.Index(_obj(users), dtype=object)

        # flatten every (method, user, position) entry, method by method
        us, it, sc, mt, rk = [], [], [], [], []
        zmean = np.zeros(len(names))
        zstd = np.zeros(len(names))
        for m, nm in enumerate(names):
            res = self.recall_results[nm]
            lens = np.fromiter((len(v) for v in res.values()), np.int64, count=len(res))
            n = int(lens.sum())
            flat = list(chain.from_iterable(res.values()))
            items = _obj([t[0] for t in flat])
            scores = np.array([t[1] for t in flat], dtype=np.float64) if n else np.zeros(0)
            us.append(np.repeat(uidx.get_indexer(_obj(list(res.keys()))), lens))
            it.append(items)
            sc.append(scores)
            mt.append(np.full(n, m, np.int32))
            rk.append((np.arange(n) - np.repeat(np.cumsum(lens) - lens, lens)).astype(np.int32))
            if NORMS.get(self.normalize_method, 0) == 2 and n:
                # fusion.py:155-175 with numpy on the host: the same mean / std
                # of the Python list and the same np.exp, so the sigmoid is the
                # reference's to the bit; the device then takes the scores as
                # pre-normalised (norm 3)
                all_scores = [t[1] for t in flat]
                mean_score = np.mean(all_scores)
                std_score = np.std(all_scores)
                if std_score > 0:
                    z = (scores - mean_score) / std_score
                    sc[-1] = 1.0 / (1.0 + np.exp(-z))
                else:
                    sc[-1] = np.full(n, 0.5)
        us = np.concatenate(us)
        if len(us) == 0:  # every list empty: {user: []} as the reference (:311-333)
            self.fused_results = {u: [] for u in users}
            return self.fused_results
        order = np.argsort(us, kind="stable")  # by user; method order, then list order inside
        item_codes, item_keys = pd.factorize(np.concatenate(it)) if len(us) else (np.zeros(0, np.int64), [])
        score = np.concatenate(sc)[order]
        counts = np.bincount(us, minlength=len(users))
        max_entries = int(counts.max(initial=0))
        if max_entries > FUSE_WIDE_MAX:
            raise NotImplementedError(f"more than {FUSE_WIDE_MAX} recalled entries for one user")
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        dev = self.device
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        t_off, t_item = d(offsets), d(item_codes[order].astype(np.int32))
        t_score, t_m = d(score), d(np.concatenate(mt)[order])
        t_rank, t_w = d(np.concatenate(rk)[order]), d(np.array([self.weights[n] for n in names], np.float64))
        norm = NORMS.get(self.normalize_method, 0)
        if norm == 2:
            norm = 3  # normalised on the host above
        gmin = gmax = 0.0
        if norm == 1 and len(score):
            mm = torch.empty(2, dtype=torch.float64, device=dev)
            call("nrk_fuse_minmax", P(t_score.data_ptr()), len(score), P(mm.data_ptr()), ops._stream())
            gmin, gmax = mm.tolist()
        seen_off = seen = None
        if remove_seen and user_history:
            code_of = pd.Index(item_keys, dtype=object) if len(item_keys) else None
            lists = [list(user_history.get(u, ())) for u in users]
            lens = np.fromiter((len(x) for x in lists), np.int64, count=len(lists))
            flat = _obj(list(chain.from_iterable(lists)))
            codes = code_of.get_indexer(flat) if code_of is not None and len(flat) else np.full(len(flat), -1)
            if len(flat):  # no history item at all (e.g. cold-start users): nothing to remove
                seen_off = d(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
                seen = d(np.where(codes >= 0, codes, -2).astype(np.int32))  # -2 never matches an item code
        strat = STRATEGIES.get(self.fusion_strategy, 1)
        o_item, o_score, o_cnt = _launch_fuse(dev, len(users), t_off, t_item, t_score, t_m, t_rank, t_w, strat, norm,
                                              gmin, gmax, d(zmean), d(zstd), seen_off, seen, max_entries, topk)
        oi, os_, oc = o_item.cpu().numpy(), o_score.cpu().numpy(), o_cnt.cpu().numpy()
        keys = np.asarray(item_keys, dtype=object)
        raw = keys[np.maximum(oi, 0)] if len(keys) else np.zeros(oi.shape, dtype=object)
        it_l, sc_l = raw.tolist(), os_.tolist()
        out = {}
        for n_, u in enumerate(users):
            c = int(oc[n_])
            out[u] = list(zip(it_l[n_][:c], sc_l[n_][:c]))
        self.fused_results = out
        return out

    # ------------------------------------------------------------------ save --
    def save(self, path: Optional[str] = None):
        """The fused dict as the pickle RecallPipeline writes
        (``all_recall_results.pkl``, recall_pipeline.py:290-294)."""
        if self.fused_results is None:
            raise ValueError("No fused results. Call fuse() first.")
        if path is None:
            path = getattr(self.config, "all_recall_results_path", None) or "all_recall_results.pkl"
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "wb") as fh:
            pickle.dump(self.fused_results, fh)
        return path


class RecallEnsemble:
    """Online counterpart of RecallFusion (fusion.py:419-556): recaller
    instances, not stored results.  The reference asks every recaller for one
    user, min-max normalises each list on its own and merges by weighted_avg,
    weighted_sum or max_score (:488-538) -- RecallFusion's local normalisation
    with three of its strategies, so the whole batch is one nrk_fuse /
    nrk_fuse_wide call (norm 0, no seen filter) with bit-identical scores."""

    def __init__(self, config=None, fusion_strategy: str = "weighted_avg", device="cuda"):
        if fusion_strategy not in ("weighted_avg", "weighted_sum", "max_score"):
            raise ValueError(f"fusion_strategy must be weighted_avg, weighted_sum or max_score, got {fusion_strategy!r}")
        self.config = config
        self.recallers: Dict[str, Dict] = {}
        self.fusion_strategy = fusion_strategy
        self.device = torch.device(device)

    def add_recaller(self, name: str, recaller, weight: float = 1.0):
        """fusion.py:446-456."""
        self.recallers[name] = {"recaller": recaller, "weight": weight}

    def _collect(self, recaller, users, k):
        """One recaller's list per user: one batch call when it has one; when
        that raises (or there is none) user by user, a failure dropping only
        that user's list from this channel (:476-483)."""
        if hasattr(recaller, "batch_recall"):
            try:
                got = recaller.batch_recall(users, k)
                return {u: got.get(u, ()) for u in users}
            except Exception:  # noqa: BLE001 -- the reference swallows any recaller failure
                pass
        out = {}
        for u in users:
            try:
                out[u] = recaller.recall(u, topk=k)
            except Exception:  # noqa: BLE001
                out[u] = ()
        return out

    def batch_recall(self, user_ids: List[int], topk: int = 10) -> Dict[int, List[Tuple[int, float]]]:
        """fusion.py:540-556 with one device merge for the whole batch."""
        users = list(dict.fromkeys(user_ids))
        if not users:
            return {}
        infos = list(self.recallers.values())
        per = [self._collect(r["recaller"], users, topk * 2) for r in infos]
        # every entry, user by user; inside a user in recaller order, then list order
        it, sc, mt, rk = [], [], [], []
        counts = np.zeros(len(users), np.int64)
        for n, u in enumerate(users):
            for m, res in enumerate(per):
                lst = res[u]
                it += [t[0] for t in lst]
                sc += [t[1] for t in lst]
                mt += [m] * len(lst)
                rk += range(len(lst))
                counts[n] += len(lst)
        if not it:
            return {u: [] for u in users}
        max_entries = int(counts.max())
        if max_entries > FUSE_WIDE_MAX:
            raise NotImplementedError(f"more than {FUSE_WIDE_MAX} recalled entries for one user")
        codes, keys = pd.factorize(_obj(it))
        weights = np.array([r["weight"] for r in infos], np.float64)
        mt = np.array(mt, np.int32)
        if self.fusion_strategy == "weighted_avg" and (weights <= 0).any():
            # the reference divides by every item's weight sum (:526-529): the sums in its order
            group = np.repeat(np.arange(len(users)), counts) * len(keys) + codes
            _, inv = np.unique(group, return_inverse=True)
            tw = np.zeros(inv.max() + 1)
            np.add.at(tw, inv, weights[mt])
            if (tw == 0).any():
                raise ZeroDivisionError("float division by zero")
            if (tw < 0).any():
                raise NotImplementedError("weighted_avg with a negative weight sum")
        dev = self.device
        d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        zero = d(np.zeros(len(infos)))
        o_item, o_score, o_cnt = _launch_fuse(
            dev, len(users), d(offsets), d(codes.astype(np.int32)), d(np.array(sc, np.float64)), d(mt),
            d(np.array(rk, np.int32)), d(weights), STRATEGIES[self.fusion_strategy], 0, 0.0, 0.0, zero, zero, None,
            None, max_entries, topk)
        oi, os_, oc = o_item.cpu().numpy(), o_score.cpu().numpy(), o_cnt.cpu().numpy()
        raw = np.asarray(keys, dtype=object)[np.maximum(oi, 0)].tolist()
        sc_l = os_.tolist()
        return {u: list(zip(raw[n][:int(oc[n])], sc_l[n][:int(oc[n])])) for n, u in enumerate(users)}

    def recall(self, user_id: int, topk: int = 10) -> List[Tuple[int, float]]:
        """fusion.py:458-538 (a batch of one)."""
        return self.batch_recall([user_id], topk)[user_id]


def _launch_fuse(dev, n_users, t_off, t_item, t_score, t_m, t_rank, t_w, strat, norm, gmin, gmax, zm, zs, seen_off,
                 seen, max_entries, topk):
    """nrk_fuse when every user has at most FUSE_MAX entries and topk fits,
    else nrk_fuse_wide -> (items [U, topk] int32, scores f64, cnt [U]) on the device."""
    o_item = torch.empty((n_users, topk), dtype=torch.int32, device=dev)
    o_score = torch.empty((n_users, topk), dtype=torch.float64, device=dev)
    o_cnt = torch.empty(n_users, dtype=torch.int32, device=dev)
    p = lambda t: P(t.data_ptr()) if t is not None else None  # noqa: E731
    n_methods = t_w.numel()
    if max_entries <= FUSE_MAX and topk <= FUSE_MAX:
        call("nrk_fuse", p(t_off), n_users, p(t_item), p(t_score), p(t_m), p(t_rank), n_methods, p(t_w), strat,
             norm, float(gmin), float(gmax), p(zm), p(zs), p(seen_off), p(seen), int(topk), p(o_item),
             p(o_score), p(o_cnt), ops._stream())
    else:
        call("nrk_fuse_wide", p(t_off), n_users, p(t_item), p(t_score), p(t_m), p(t_rank), n_methods, p(t_w),
             strat, norm, float(gmin), float(gmax), p(zm), p(zs), p(seen_off), p(seen), max_entries, int(topk),
             p(o_item), p(o_score), p(o_cnt), ops._stream())
    return o_item, o_score, o_cnt


def _obj(seq):
    a = np.empty(len(seq), dtype=object)
    a[:] = seq
    return a

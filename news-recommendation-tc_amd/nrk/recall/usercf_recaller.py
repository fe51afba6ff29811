"""UserCF recaller: drop-in for src/recall/usercf_recaller.py:10-118.

``recall`` / ``batch_recall`` run on the GPU (nrk_usercf_recall: every query
user of a batch in one call -- the walk over (neighbour rank, position in the
neighbour's history) with its position, content and created-time weights,
then ItemCF's back end: ordered per-(user, item) sums through a stable radix
sort, hot-item fill and the stable top-k).  Each user's stable top
``usercf_sim_user_topk`` neighbours come from UserCFSimilarity.compute()'s
device result (``from_result``) or, given the reference's u2u dict, from
nrk_itemcf_topn, as ItemCFRecaller takes its item neighbours.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

from .. import ops
from .base import BaseRecaller

CREATED_ALPHA = 0.8  # the literal alpha of usercf_recaller.py:96-100 (not created_time_alpha)


class UserCFRecaller(BaseRecaller):
    def __init__(self, config, similarity_matrix: Dict, user_item_time_dict: Dict, item_created_time_dict: Dict,
                 item_topk_click: List, emb_similarity_matrix: Dict = None, device="cuda", sim_result=None):
        super().__init__(config)
        self.u2u_sim = similarity_matrix
        self.user_item_time_dict = user_item_time_dict
        self.item_created_time_dict = item_created_time_dict
        self.item_topk_click = item_topk_click
        self.emb_i2i_sim = emb_similarity_matrix or {}
        self.device = torch.device(device)
        self._sim_result = sim_result
        self._build()

    @classmethod
    def from_result(cls, config, sim_result, user_item_time_dict, item_created_time_dict, item_topk_click,
                    emb_similarity_matrix=None, device="cuda"):
        """Build straight from UserCFSimilarity.compute()'s device top-n (no u2u dict)."""
        return cls(config, None, user_item_time_dict, item_created_time_dict, item_topk_click,
                   emb_similarity_matrix, device, sim_result)

    def _top_neighbours(self):
        """-> (raw ids of the rows, raw neighbour ids [R, topn], vals [R, topn], cnt [R]):
        sorted(u2u_sim[u].items(), key=sim, reverse=True)[:usercf_sim_user_topk] (:59-62)."""
        topn = self.config.usercf_sim_user_topk
        if self._sim_result is not None:
            r = self._sim_result
            oc, ov = r.top(topn)
            oc, ov = oc.cpu().numpy(), ov.cpu().numpy()
            cnt = np.minimum(r.nnz.cpu().numpy(), topn).astype(np.int32)
            return r.user_ids, r.user_ids[np.maximum(oc, 0)], ov, cnt
        rows = list(self.u2u_sim.keys())
        lens = np.array([len(self.u2u_sim[u]) for u in rows], np.int64)
        off = np.zeros(len(rows) + 1, np.int64)
        off[1:] = np.cumsum(lens)
        n = int(off[-1])
        if n >= 2**31:
            raise ValueError("similarity has >= 2^31 entries")
        vs_ = np.empty(n, np.int64)
        ws_ = np.empty(n, np.float64)
        k = 0
        for u in rows:
            sd = self.u2u_sim[u]
            m = len(sd)
            vs_[k:k + m] = list(sd.keys())
            ws_[k:k + m] = list(sd.values())
            k += m
        d = self.device
        pos = torch.arange(n, dtype=torch.int32, device=d)
        oc, _, cnt = ops.itemcf_topn(torch.from_numpy(off).to(d), pos, torch.from_numpy(ws_).to(d),
                                     pos.to(torch.int64), topn)
        oc, cnt = oc.cpu().numpy(), cnt.cpu().numpy()
        sel = np.maximum(oc, 0)
        return (np.asarray(rows, np.int64).reshape(-1), vs_[sel] if n else np.zeros(oc.shape, np.int64),
                ws_[sel] if n else np.zeros(oc.shape), cnt)

    def _build(self):
        """Dense user rows = user_item_time_dict order, dense item ids over every
        item of a history or the hot list, and the device arrays of the recall."""
        d = self.device
        rows_raw, cols_raw, vals, cnt = self._top_neighbours()
        topn = max(cols_raw.shape[1], 1) if cols_raw.ndim == 2 else 1
        users = list(self.user_item_time_dict.keys())
        n_users = len(users)
        slot = {u: k for k, u in enumerate(users)}
        lens = np.fromiter((len(self.user_item_time_dict[u]) for u in users), np.int64, n_users)
        offs = np.zeros(n_users + 1, np.int64)
        offs[1:] = np.cumsum(lens)
        hist = np.fromiter((it for u in users for it, _ in self.user_item_time_dict[u]), np.int64, int(offs[-1]))
        hot = np.asarray(list(self.item_topk_click), np.int64)
        ids = np.unique(np.concatenate([hist, hot]))
        n_items = max(len(ids), 1)
        # neighbour rows: a neighbour without a history is skipped (:67-68), the others keep their order
        nb_cols = np.full((max(n_users, 1), topn), -1, np.int32)
        nb_vals = np.zeros((max(n_users, 1), topn), np.float64)
        nb_cnt = np.zeros(max(n_users, 1), np.int32)
        self._known = set()
        for r, u in enumerate(rows_raw.tolist()):
            self._known.add(u)
            k = slot.get(u)
            m = int(cnt[r])
            if k is None or m == 0:
                continue
            nb = [(slot[v], w) for v, w in zip(cols_raw[r, :m].tolist(), vals[r, :m].tolist()) if v in slot]
            nb_cnt[k] = len(nb)
            if nb:
                nb_cols[k, :len(nb)] = [a for a, _ in nb]
                nb_vals[k, :len(nb)] = [b for _, b in nb]
        # loc_weight = 1.0 + sum_loc beta ** (L - loc), summed in loc order (:77-86):
        # Python's float ** int per distance, a sequential cumsum per history length
        beta = float(self.config.loc_beta)
        max_len = int(lens.max()) if n_users else 0
        pw = [beta ** dist for dist in range(max_len + 1)]
        by_len = {}
        for L in np.unique(lens).tolist():
            by_len[L] = float(np.cumsum(np.array([1.0] + pw[L:0:-1], np.float64))[-1])
        loc_w = np.fromiter((by_len[L] for L in lens.tolist()), np.float64, n_users)
        # created times: the walk reads created[i] for the clicks i of a user's
        # neighbours and created[j] for that user's own history (:96-100); a
        # missing one is the reference's KeyError
        ct = self.item_created_time_dict
        created = np.fromiter((float(ct.get(int(x), np.nan)) for x in ids), np.float64, len(ids))
        hist_rows = np.searchsorted(ids, hist) if len(hist) else np.zeros(0, np.int64)
        reads = np.zeros(max(n_users, 1), bool)
        reads[:n_users] = nb_cnt[:n_users] > 0
        valid = np.arange(topn)[None, :] < nb_cnt[:, None]
        reads[nb_cols[valid]] = True
        looked = np.zeros(len(ids), bool)
        looked[hist_rows[np.repeat(reads[:n_users], lens)]] = True
        missing = looked & np.isnan(created)
        if missing.any():
            raise KeyError(int(ids[np.argmax(missing)]))
        created = np.where(np.isnan(created), 0.0, created)  # hot-fill only items: never read
        self._ids = ids
        self._slot = slot
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)  # noqa: E731
        self._dev = {
            "offsets": t(offs), "items": t(hist_rows.astype(np.int32)),
            "nbr_cols": t(nb_cols[:n_users]), "nbr_vals": t(nb_vals[:n_users]), "nbr_cnt": t(nb_cnt[:n_users]),
            "loc_w": t(loc_w), "created": t(created if len(ids) else np.zeros(1)),
            "hot": t(np.searchsorted(ids, hot).astype(np.int32)),
        }
        self._emb = None
        if self.emb_i2i_sim:
            pos = {int(x): k for k, x in enumerate(ids)}
            rows = {}
            for i, dd in self.emb_i2i_sim.items():
                pi = pos.get(i)
                if pi is None:
                    continue
                rows[pi] = [(pos[j], v) for j, v in dd.items() if j in pos]
            ke = max([len(r) for r in rows.values()] + [1])
            ec = np.full((n_items, ke), -1, np.int32)
            ev = np.zeros((n_items, ke), np.float64)
            en = np.zeros(n_items, np.int32)
            for pi, r in rows.items():
                en[pi] = len(r)
                if r:
                    ec[pi, :len(r)] = [a for a, _ in r]
                    ev[pi, :len(r)] = [b for _, b in r]
            self._emb = (t(ec), t(ev), t(en))

    def batch_recall(self, user_ids: List[int], topk: int = 10) -> Dict[int, List[Tuple[int, float]]]:
        """Every user of the batch in one nrk_usercf_recall call."""
        user_ids = list(user_ids)
        if not user_ids:
            return {}
        dv = self._dev
        # cold start: no history, or no u2u row (:49-53)
        q = torch.tensor([self._slot.get(u, -1) if u in self._known else -1 for u in user_ids], dtype=torch.int64,
                         device=self.device)
        e = self._emb or (None, None, None)
        oi, osc, osrc, ocnt = ops.usercf_recall(q, dv["offsets"], dv["items"], dv["nbr_cols"], dv["nbr_vals"],
                                                dv["nbr_cnt"], dv["loc_w"], dv["created"], dv["hot"], topk,
                                                CREATED_ALPHA, *e)
        oi, osc, osrc, ocnt = (x.cpu().numpy() for x in (oi, osc, osrc, ocnt))
        ids = self._ids
        out = {}
        for n, u in enumerate(user_ids):
            m = int(ocnt[n])
            raw = ids[oi[n, :m]].tolist()
            sc = osc[n, :m].tolist()
            src = osrc[n, :m].tolist()
            # hot-fill / cold-start scores are Python ints in the reference (:50, :109)
            out[u] = [(it, float(v) if k == 0 else int(v)) for it, v, k in zip(raw, sc, src)]
        return out

    def recall(self, user_id: int, topk: int = 10) -> List[Tuple[int, float]]:
        """usercf_recaller.py:37-118 on the GPU (a batch of one)."""
        return self.batch_recall([user_id], topk)[user_id]

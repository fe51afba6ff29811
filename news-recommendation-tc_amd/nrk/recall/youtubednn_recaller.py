"""GPU YouTubeDNN recaller: drop-in for src/recall/youtubednn_recaller.py.

Same plugin contract as the reference's ``YoutubeDNNRecaller``
(youtubednn_recaller.py:191-569): raw user ids in, ``[(raw_item_id, score)]``
out, rank 0 of the (topk+1) search dropped (:524), Faiss row r mapped through
``item_index_2_rawid[r]`` (:528-529 -- the reference's row->id quirk is kept
on purpose), unknown users -> ``[]`` (:513-514), not
ready -> ``ValueError`` (:508-509).

What changes is underneath: the user/item towers run as HIP kernels
(nrk_tt_user_fwd / nrk_tt_item_fwd), the Faiss IndexFlatIP becomes a device
catalog (nrk_ip_catalog_build) and ``batch_recall`` is ONE device top-k call
for the whole user list instead of one Faiss search per user: nrk_ip_topk, or,
up to ``query_max_users`` users (``recall(user_id)`` is one), nrk_ip_query,
which splits the catalog across the chip instead of the users.
``train`` (:211-423) runs on the GPU as well: the samples are generated on the
device (nrk_tt_make_samples), every step is one fused forward + loss +
backward (nrk_tt_train_grad) and one dense-semantics Adam sweep
(nrk_tt_adam_step), with no host synchronisation between steps; it ends
through ``load_model``.  Weights trained elsewhere still load with
``load_model``, precomputed embeddings with ``from_embeddings``.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import pandas as pd
import torch

from .. import ops
from ..config import RecallConfig
from ..data import extractors
from .base import BaseRecaller


def _as_mapping_array(m, n=None):
    if isinstance(m, dict):
        n = len(m) if n is None else n
        return np.array([m[i] for i in range(n)], dtype=np.int64)
    return np.asarray(m, dtype=np.int64)


class YoutubeDNNRecaller(BaseRecaller):
    # batch_recall searches with ops.ip_query up to this many known users (and
    # topk + 1 <= 128), with ops.ip_topk above; 0 = always ip_topk.  An instance
    # may override it.  From profiles/r10_query.txt (tools/query_bench.py), the
    # line "config-2 catalog: largest n_users with every ip_query run below
    # every ip_topk run = 512", halved for catalogs of other sizes and dims.
    query_max_users = 256

    def __init__(self, config: RecallConfig | None = None, device: str | torch.device = "cuda"):
        super().__init__(config or RecallConfig())
        self.seq_max_len = getattr(self.config, "youtubednn_seq_max_len", 30)
        self.embedding_dim = getattr(self.config, "youtubednn_embedding_dim", 16)
        self.hidden_units = getattr(self.config, "youtubednn_hidden_units", [64, 16])
        self.device = torch.device(device)
        self.user_index_2_rawid: Dict[int, int] = {}
        self.user_rawid_2_index: Dict[int, int] = {}
        self.item_index_2_rawid: Dict[int, int] = {}
        self.item_rawid_2_index: Dict[int, int] = {}
        self.user_embeddings = None  # torch [U, D] on device
        self.item_embeddings = None  # torch [I, D] on device
        self.catalog = None          # ops.Catalog = the Faiss index
        self._item_raw = None        # np [I] row -> raw id (quirk mapping)
        self.negsample = int(getattr(self.config, "youtubednn_negsample", 4))
        self.dropout = 0.2           # nn.Dropout(0.2) after every layer (:110)
        self._trained = None         # (user table, item table, packed weights, widths) after training
        self.epoch_losses: List[float] = []

    # -------------------------------------------------------------- setup --
    @classmethod
    def from_embeddings(cls, user_embeddings, item_embeddings, user_index_2_rawid,
                        item_index_2_rawid, config=None, device="cuda"):
        """Wrap already-extracted embeddings (the state after
        _extract_embeddings, youtubednn_recaller.py:425-495)."""
        self = cls(config, device)
        dev = lambda x: (x.to(self.device, torch.float32) if torch.is_tensor(x)  # noqa: E731
                         else torch.as_tensor(np.asarray(x, np.float32)).to(self.device)).contiguous()
        ue, ie = dev(user_embeddings), dev(item_embeddings)
        self._set_state(ue, ie, _as_mapping_array(user_index_2_rawid),
                        _as_mapping_array(item_index_2_rawid))
        return self

    def load_model(self, state_dict, click_df):
        """Build mappings exactly as train() does (label encoding :324-353),
        then run both towers on the GPU for every user / item
        (_extract_embeddings :425-495).  ``state_dict`` holds the reference
        module's parameters (user_embedding.weight, item_embedding.weight,
        user_tower.0.*, user_tower.3.*)."""
        sd = {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v))
              for k, v in state_dict.items()}
        # user_tower = [Linear, ReLU, Dropout] per hidden unit: Linear l at index 3 l (:105-112)
        n_layers = len([k for k in sd if k.startswith("user_tower.") and k.endswith(".weight")])
        user_col = np.asarray(click_df["user_id"], np.int64)
        uid, hist, hlen, item_raw, profile = extractors.youtubednn_histories(
            user_col, np.asarray(click_df["click_article_id"], np.int64), self.seq_max_len)
        user_raw = np.unique(user_col)
        dev = self.device
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        tabs = (f(sd["user_embedding.weight"].astype(np.float32)), f(sd["item_embedding.weight"].astype(np.float32)),
                f(uid.astype(np.int32)), f(hist.astype(np.int32)), f(hlen.astype(np.int32)))
        layers = [(f(sd[f"user_tower.{3 * l}.weight"].astype(np.float32)),
                   f(sd[f"user_tower.{3 * l}.bias"].astype(np.float32))) for l in range(n_layers)]
        if n_layers == 2 and layers[0][0].shape[0] <= 128:  # the tuned two-layer kernel (LDS-resident weights)
            ue = ops.tt_user_fwd(*tabs, *layers[0], *layers[1])
        else:
            ue = ops.tt_user_fwd_layers(*tabs, layers)
        ie = ops.tt_item_fwd(f(sd["item_embedding.weight"].astype(np.float32)),
                             f(profile.astype(np.int32)))
        self._set_state(ue, ie, user_raw, item_raw)
        return self

    # ----------------------------------------------------------- training --
    def train(self, click_df, epochs: int = 1, batch_size: int = 256, learning_rate: float = 0.001, seed=None):
        """YoutubeDNNRecaller.train (:312-423) on the GPU.  Label encoding as
        load_model's (:324-353); _prepare_data's samples (:230-300) made on the
        device from the time-ordered click log, negatives uniform over the
        log's items, shuffled by a device permutation before every epoch (the
        DataLoader's shuffle=True); _init_weights' initialisation (:119-127);
        BCEWithLogitsLoss + Adam(lr) (:381-412).  ``seed`` (default
        config.random_seed) fixes the initialisation, the negatives, the
        shuffles and the dropout masks: two runs with one seed are
        bit-identical.  Prints the average loss per epoch and finishes through
        load_model, so recall / batch_recall work afterwards."""
        seed = int(getattr(self.config, "random_seed", 23) if seed is None else seed)
        user_col = np.asarray(click_df["user_id"], np.int64)
        item_col = np.asarray(click_df["click_article_id"], np.int64)
        ts = np.asarray(click_df["click_timestamp"], np.int64)
        u_classes, u_enc = np.unique(user_col, return_inverse=True)
        i_classes, i_enc = np.unique(item_col, return_inverse=True)
        # sort_values("click_timestamp") then groupby user (:230, :248); equal stamps keep their row order
        order = np.lexsort((np.arange(len(ts)), ts, u_enc))
        log_off = np.concatenate([[0], np.cumsum(np.bincount(u_enc, minlength=len(u_classes)))]).astype(np.int64)
        dev = self.device
        log_off_d = torch.as_tensor(log_off).to(dev)
        log_items_d = torch.as_tensor(i_enc[order].astype(np.int32)).to(dev)
        pool = torch.arange(len(i_classes), dtype=torch.int32, device=dev)  # click_article_id.unique() (:233)
        state = self.init_state(len(u_classes), len(i_classes), seed)
        samples = ops.tt_make_samples(log_off_d, log_items_d, self.negsample, pool, seed)
        if not samples[0].numel():
            raise ValueError("no training samples: every user has fewer than 3 clicks")
        print("Training YoutubeDNN model...")
        self.train_on_samples(state, log_off_d, log_items_d, *samples, batch_size=batch_size, epochs=epochs,
                              learning_rate=learning_rate, dropout=self.dropout, seed=seed, shuffle=True, verbose=True)
        self.load_model(self.state_dict(), click_df)
        print("Training completed!")
        return self

    def init_state(self, n_users: int, n_items: int, seed: int = 0):
        """YoutubeDNN._init_weights (:119-127): xavier-uniform Linear weights,
        zero biases, N(0, 0.01) embeddings, under the reference's key names."""
        g = torch.Generator().manual_seed(int(seed))
        D = self.embedding_dim
        sd = {"user_embedding.weight": torch.empty(n_users, D).normal_(0.0, 0.01, generator=g),
              "item_embedding.weight": torch.empty(n_items, D).normal_(0.0, 0.01, generator=g)}
        fan_in = 2 * D
        for l, w in enumerate(self.hidden_units):
            a = (6.0 / (fan_in + w)) ** 0.5
            sd[f"user_tower.{3 * l}.weight"] = torch.empty(w, fan_in).uniform_(-a, a, generator=g)
            sd[f"user_tower.{3 * l}.bias"] = torch.zeros(w)
            fan_in = w
        return sd

    def train_on_samples(self, state_dict, log_off, log_items, s_user, s_pos, s_target, s_label,
                         batch_size: int = 256, epochs: int = 1, learning_rate: float = 0.001,
                         dropout: float = 0.2, seed: int = 0, shuffle: bool = False, verbose: bool = False):
        """The training loop over explicit samples from an initial state_dict
        (the reference module's keys): consecutive batches of ``batch_size``
        (the last one short, drop_last=False), every epoch in the given order
        unless ``shuffle``.  Returns the per-step losses (fp32, on the host,
        read from the device once per epoch); the trained parameters are then
        in ``state_dict()``."""
        dev = self.device
        t32 = lambda a, dt: (a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))).to(dev, dt).contiguous()  # noqa: E731
        log_off, log_items = t32(log_off, torch.int64), t32(log_items, torch.int32)
        s_user, s_pos, s_target = (t32(a, torch.int32) for a in (s_user, s_pos, s_target))
        s_label = t32(s_label, torch.float32)
        sd = {k: t32(v.detach() if torch.is_tensor(v) else v, torch.float32) for k, v in state_dict.items()}
        n_layers = len([k for k in sd if k.startswith("user_tower.") and k.endswith(".weight")])
        ue, ie = sd["user_embedding.weight"].clone(), sd["item_embedding.weight"].clone()
        weights, widths = ops.tt_pack_layers([(sd[f"user_tower.{3 * l}.weight"], sd[f"user_tower.{3 * l}.bias"])
                                              for l in range(n_layers)])
        moments = [torch.zeros_like(x) for x in (weights, weights, ue, ue, ie, ie)]
        n, T, D = s_user.numel(), self.seq_max_len, ue.shape[1]
        if not 1 <= batch_size <= ops.TT_MAX_BATCH:
            raise ValueError(f"batch_size must be in [1, {ops.TT_MAX_BATCH}]")
        if n == 0:
            raise ValueError("no samples")
        bounds = [(a, min(n, a + batch_size)) for a in range(0, n, batch_size)]
        bufs = {b - a: ops.TtGrads(dev, b - a, T, D, weights.numel()) for a, b in (bounds[0], bounds[-1])}
        # every index is range-checked here, once, so that no step synchronises with the host
        if log_off.shape[0] != ue.shape[0] + 1:
            raise ValueError("log_off must have one row per user of the user table")
        ops.tt_check_samples(ue.shape[0], ie.shape[0], log_off, log_items, s_user, s_pos, s_target, T)
        gen = torch.Generator(device=dev).manual_seed(int(seed)) if shuffle else None
        all_losses, step = [], 0
        self.epoch_losses = []
        for epoch in range(epochs):
            cur = (s_user, s_pos, s_target, s_label)
            if shuffle:
                perm = torch.randperm(n, device=dev, generator=gen)
                cur = tuple(a[perm].contiguous() for a in cur)
            losses = torch.zeros(len(bounds), dtype=torch.float32, device=dev)
            for s, (a, b) in enumerate(bounds):
                g = ops.tt_train_grad(ue, ie, weights, widths, log_off, log_items, cur[0][a:b], cur[1][a:b],
                                      cur[2][a:b], cur[3][a:b], T, p=dropout, seed=seed, step=step,
                                      validate=False, out=bufs[b - a], loss=losses[s:s + 1])
                ops.tt_adam_step(weights, moments[0], moments[1], ue, moments[2], moments[3], ie, moments[4],
                                 moments[5], g, t=step + 1, lr=learning_rate)
                step += 1
            host = losses.cpu()  # the epoch's one read of the device
            all_losses.append(host)
            self.epoch_losses.append(float(host.double().mean()))
            if verbose:
                print(f"Epoch {epoch + 1} - Avg Loss: {self.epoch_losses[-1]:.4f}")
        self._trained = (ue, ie, weights, widths)
        return torch.cat(all_losses)

    def state_dict(self):
        """The trained parameters under the reference module's key names (host
        tensors): loads into the reference's YoutubeDNN and into load_model."""
        if self._trained is None:
            raise ValueError("Model not trained. Call train() first.")
        ue, ie, weights, widths = self._trained
        sd = {"user_embedding.weight": ue.cpu(), "item_embedding.weight": ie.cpu()}
        for l, (w, b) in enumerate(ops.tt_unpack_layers(weights, widths, ue.shape[1])):
            sd[f"user_tower.{3 * l}.weight"] = w.cpu().clone()
            sd[f"user_tower.{3 * l}.bias"] = b.cpu().clone()
        return sd

    def _set_state(self, ue, ie, user_raw, item_raw):
        self.user_embeddings = ue
        self.item_embeddings = ie
        self.user_index_2_rawid = {i: int(r) for i, r in enumerate(user_raw)}
        self.user_rawid_2_index = {int(r): i for i, r in enumerate(user_raw)}
        self.item_index_2_rawid = {i: int(r) for i, r in enumerate(item_raw)}
        self.item_rawid_2_index = {int(r): i for i, r in enumerate(item_raw)}
        self._item_raw = np.asarray(item_raw, np.int64)
        self._user_index = pd.Index(np.asarray(user_raw, np.int64))
        self.catalog = ops.Catalog(ie)

    # ------------------------------------------------------------- recall --
    def recall(self, user_id: int, topk: int = 20) -> List[Tuple[int, float]]:
        return self.batch_recall([user_id], topk)[user_id]

    def batch_recall(self, user_ids: List[int], topk: int = 20) -> Dict[int, List[Tuple[int, float]]]:
        """BaseRecaller.batch_recall (recall/base.py:24-40) as ONE device
        top-(k+1) search; the result dict is built with vectorised id mapping
        (row r -> item_index_2_rawid[r], the reference's quirk) and one
        zip per user instead of a per-item Python loop."""
        if self.user_embeddings is None or self.catalog is None:
            raise ValueError("Model not trained. Call train() first.")
        n_users = self.user_embeddings.shape[0]
        arr = np.asarray(user_ids)
        # the int64 index path only where the cast is value-preserving: signed
        # ids, or unsigned ids below 2^63 (a larger uint64 would wrap onto
        # another user); everything else takes the dict lookup
        fits = arr.dtype.kind == "i" or (arr.dtype.kind == "u" and (arr.size == 0 or int(arr.max()) < 2 ** 63))
        if fits and arr.ndim == 1 and self._user_index.is_unique:
            idx = self._user_index.get_indexer(arr.astype(np.int64))
        else:  # str / float / mixed ids: the reference's own dict lookup (user_rawid_2_index.get, :511)
            idx = np.array([self.user_rawid_2_index.get(u, -1) for u in user_ids], np.int64)
        known = (idx >= 0) & (idx < n_users)
        results: Dict[int, List[Tuple[int, float]]] = dict.fromkeys(user_ids)
        for u in results:
            results[u] = []
        if not known.any():
            return results
        rows_needed = torch.as_tensor(idx[known], device=self.device)
        q = self.user_embeddings.index_select(0, rows_needed).contiguous()
        if q.shape[0] <= min(self.query_max_users, ops.IP_QUERY_MAX_USERS) and topk + 1 <= ops.IP_QUERY_KMAX:
            s, r = ops.ip_query(q, self.catalog, topk + 1)  # few users: the catalog-split search
        else:
            s, r = ops.ip_topk(q, self.catalog, topk + 1)
        s = s[:, 1:].cpu().numpy()  # rank 0 dropped (youtubednn_recaller.py:524)
        r = r[:, 1:].cpu().numpy().astype(np.int64)
        n_map = len(self._item_raw)
        ok = (r >= 0) & (r < n_map)
        items = self._item_raw[np.where(ok, r, 0)]
        kn = [u for u, k in zip(user_ids, known) if k]
        full = ok.all(1)
        it_l, sc_l = items.tolist(), s.tolist()
        if full.all():
            results.update(zip(kn, map(list, map(zip, it_l, sc_l))))
        else:
            for n, u in enumerate(kn):
                if full[n]:
                    results[u] = list(zip(it_l[n], sc_l[n]))
                else:  # -1 padding (fewer than topk + 1 items): skipped like :528
                    results[u] = [(it_l[n][i], sc_l[n][i]) for i in range(topk) if ok[n, i]]
        return results

    def construct_embedding_dict(self, save: bool = False):
        if self.user_embeddings is None or self.item_embeddings is None:
            raise ValueError("Embeddings not extracted. Call train() first.")
        ue = self.user_embeddings.cpu().numpy()
        ie = self.item_embeddings.cpu().numpy()
        user_emb_dict = {self.user_index_2_rawid[i]: ue[i] for i in range(len(ue))}
        item_emb_dict = {self.item_index_2_rawid[i]: ie[i] for i in range(len(ie))}
        if save:
            import os
            import pickle

            os.makedirs(self.config.save_path, exist_ok=True)
            for name, obj in (("user_youtubednn_emb.pkl", user_emb_dict),
                              ("article_youtubednn_emb.pkl", item_emb_dict)):
                with open(os.path.join(self.config.save_path, name), "wb") as fh:
                    pickle.dump(obj, fh)
        return user_emb_dict, item_emb_dict

"""User profiles, item features and labels on the GPU.

Restates three methods of the reference's feature pipeline
(src/features/feature_extractor.py) over a click log resident on the device:
  * _extract_user_profile_features (:296-389): per user the MinMax-scaled
    click count, average time gap and mean click time, the device-group mode
    and the mean word count of the distinct clicked articles;
  * _extract_item_features (:391-438): per article row its category, MinMax
    popularity (fitted over clicked articles; 0.0 when unclicked), creation
    time and word count;
  * _add_labels (:752-836): 1 where a recalled item is the user's last click;
and the label encoding of the two dicts that DINRanker._prepare_vocab_dicts
(src/rank/DIN.py:579-603) fits: the code of a value is 1 + its rank among the
column's distinct values.

Two quirks of the reference are part of its output:
  * load_data re-keys article_words_dict by ``str`` (:110-112) and the
    profile loop looks it up with integer ids (:353): every lookup misses and
    avg_word_count is 0.0 for every user.  ``repair_word_lookup=False`` (the
    default) reproduces that, ``True`` uses the real table.
  * the profile dict is filled from ``iterrows`` over a numeric frame, so the
    device group is stored as ``str`` of a float ("1.0", "10.0", ...), and
    LabelEncoder sorts those strings: "10.0" comes before "2.0".
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops

USER_FEATURES = ["user_click_count", "user_avg_time_gap", "device_group", "avg_click_time", "avg_word_count"]
ITEM_FEATURES = ["category_id", "article_popularity", "created_at_ts", "words_count"]


def _rank_codes(col):
    """1 + dense rank among the distinct values, and the vocabulary size."""
    uniq, inv = torch.unique(col, sorted=True, return_inverse=True)
    return (inv + 1).to(torch.int32), int(uniq.numel()) + 1


class ProfileFeatures:
    """See the module doc.  Build with ``from_frames`` or ``from_device``."""

    @classmethod
    def from_frames(cls, train_click_df, article_info_df, device="cuda", repair_word_lookup=False):
        """The reference's two frames (user_id, click_article_id,
        click_timestamp, click_deviceGroup; click_article_id, category_id,
        created_at_ts, words_count) -> the CSR and the dense id maps, once.
        Users are the groupby's: ascending user_id; item rows are the
        article frame's rows; a clicked article without an article row gets
        a row past the table (distinct, 0 words, counted by the popularity
        fit as the reference's value_counts does)."""
        import pandas as pd

        uid = train_click_df["user_id"].to_numpy()
        user_ids, urow = np.unique(uid, return_inverse=True)
        order = np.argsort(urow, kind="stable")  # frame order inside a user
        u_off = np.concatenate([[0], np.cumsum(np.bincount(urow, minlength=len(user_ids)))]).astype(np.int64)
        item_ids = article_info_df["click_article_id"].to_numpy()
        index = pd.Index(item_ids)
        if not index.is_unique:
            raise ValueError("article_info_df lists an article twice")
        aid = train_click_df["click_article_id"].to_numpy()[order]
        irow = index.get_indexer(aid)
        miss = irow < 0
        extra, extra_ids = pd.factorize(aid[miss])
        irow[miss] = len(item_ids) + extra
        n_rows = len(item_ids) + len(extra_ids)
        dev_values, dcode = np.unique(train_click_df["click_deviceGroup"].to_numpy()[order], return_inverse=True)
        if not np.issubdtype(dev_values.dtype, np.number):
            raise TypeError("click_deviceGroup must be numeric")
        d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
        self = cls.from_device(
            d(u_off, np.int64), d(irow, np.int32), d(train_click_df["click_timestamp"].to_numpy()[order], np.int64),
            d(dcode, np.int32), dev_values, d(article_info_df["category_id"].to_numpy(), np.int64),
            d(article_info_df["created_at_ts"].to_numpy(), np.int64),
            d(article_info_df["words_count"].to_numpy(), np.int64), n_rows=n_rows, user_ids=user_ids,
            item_ids=item_ids, repair_word_lookup=repair_word_lookup)
        self.row_ids = np.concatenate([item_ids, np.asarray(extra_ids, dtype=item_ids.dtype)])
        return self

    @classmethod
    def from_device(cls, u_off, item, ts, dev_code, dev_values, category, created, words, n_rows=None,
                    user_ids=None, item_ids=None, repair_word_lookup=False, validate=True):
        """Tensors already laid out (include/nrk.h: nrk_profile_user):
        u_off [U + 1] int64; per click item row int32, timestamp int64 and
        device-group code int32, inside a user in frame order; ``dev_values``
        the raw device-group value of every code, ascending (host; more than
        64 raise NotImplementedError); the article columns int64 [I].  Item rows lie in [0, n_rows),
        n_rows >= I.  ``user_ids`` / ``item_ids``: the raw ids of the rows for
        ``dicts()`` (default: the row numbers)."""
        self = cls.__new__(cls)
        dev_values = np.asarray(dev_values)
        if len(dev_values) > 1 and not bool((dev_values[1:] > dev_values[:-1]).all()):
            raise ValueError("dev_values must be strictly ascending")
        n_items = category.numel()
        ops._need(category, torch.int64, (n_items,), "category")
        ops._need(created, torch.int64, (n_items,), "created")
        ops._need(words, torch.int64, (n_items,), "words")
        n_rows = n_items if n_rows is None else int(n_rows)
        U = u_off.numel() - 1
        self.n_users, self.n_items, self.n_rows = U, n_items, n_rows
        self.dev_values = dev_values
        self.user_ids = np.arange(U) if user_ids is None else np.asarray(user_ids)
        self.item_ids = np.arange(n_items) if item_ids is None else np.asarray(item_ids)
        if len(self.user_ids) != U or len(self.item_ids) != n_items:
            raise ValueError("user_ids / item_ids must name every row")
        self.row_ids = self.item_ids  # raw id of every item row; from_frames appends the rows past the table
        self.repair_word_lookup = bool(repair_word_lookup)
        # the shipped lookup misses every article: an empty words table
        table = words if repair_word_lookup else words[:0]
        cnt, gap, mean_ts, mode, mean_words, last = ops.profile_user(u_off, item, ts, dev_code, len(dev_values), table,
                                                                     n_rows, validate=validate)
        if U and bool((cnt == 0).any()):
            raise ValueError("every user row needs at least one click")
        self.last_item = last
        self.user_raw = {
            "click_count": cnt, "avg_time_gap": gap, "mean_click_time": mean_ts, "device_code": mode,
            "user_click_count": ops.profile_minmax_scale(cnt.to(torch.float64)),
            "user_avg_time_gap": ops.profile_minmax_scale(gap),
            "avg_click_time": ops.profile_minmax_scale(mean_ts),
            "avg_word_count": mean_words,
        }
        pop = ops.profile_item_count(item, n_rows).to(torch.float64)
        self.item_raw = {
            "click_count": pop[:n_items].to(torch.int64),
            "category_id": category,
            "article_popularity": ops.profile_minmax_scale(pop, fit=pop[pop > 0], skip_zero=True)[:n_items].contiguous(),
            "created_at_ts": created,
            "words_count": words,
        }
        return self

    # --------------------------------------------------------------- outputs --
    def _device_strs(self):
        """``str(row["device_group"])`` of every code: the row is float64."""
        return [str(np.float64(v)) for v in self.dev_values]

    def dicts(self):
        """(user_profile_dict, item_features_dict, user_profile_features,
        item_features) as the reference builds them: keys, key order, value
        types."""
        ur, ir = self.user_raw, self.item_raw
        host = lambda t: t.cpu().tolist()  # noqa: E731
        strs = self._device_strs()
        user = {}
        for u, c, g, m, t, w in zip(self.user_ids.tolist(), host(ur["user_click_count"]),
                                    host(ur["user_avg_time_gap"]), host(ur["device_code"]),
                                    host(ur["avg_click_time"]), host(ur["avg_word_count"])):
            user[str(int(u))] = {"user_click_count": c, "user_avg_time_gap": g, "device_group": strs[m],
                                 "avg_click_time": t, "avg_word_count": w}
        items = {}
        for i, c, p, t, w in zip(self.item_ids.tolist(), host(ir["category_id"]), host(ir["article_popularity"]),
                                 host(ir["created_at_ts"]), host(ir["words_count"])):
            items[str(i)] = {"category_id": c, "article_popularity": p, "created_at_ts": t, "words_count": w}
        return user, items, list(USER_FEATURES), list(ITEM_FEATURES)

    def encoded(self):
        """(user_table int32 [U, 5], item_table int32 [I, 4], user vocabulary
        sizes, item vocabulary sizes): DinEncoder's tables under the encoders
        of _prepare_vocab_dicts, in USER_FEATURES / ITEM_FEATURES order."""
        ur, ir = self.user_raw, self.item_raw
        dev = self.last_item.device
        # device_group: LabelEncoder over the str forms of the modes that occur, sorted as strings
        present = torch.unique(ur["device_code"]).cpu().tolist()
        strs = self._device_strs()
        order = sorted(present, key=lambda c: strs[c])
        lut = np.zeros(max(len(strs), 1), np.int32)
        for rank, c in enumerate(order):
            lut[c] = rank + 1
        dcode = torch.from_numpy(lut).to(dev)[ur["device_code"].long()]
        ucols, uvoc = [], []
        for f in USER_FEATURES:
            if f == "device_group":
                col, v = dcode, len(order) + 1
            else:
                col, v = _rank_codes(ur[f])
            ucols.append(col)
            uvoc.append(v)
        icols, ivoc = [], []
        for f in ITEM_FEATURES:
            col, v = _rank_codes(ir[f])
            icols.append(col)
            ivoc.append(v)
        return torch.stack(ucols, 1).contiguous(), torch.stack(icols, 1).contiguous(), uvoc, ivoc

    def labels(self, user_rows, item_rows, offline=True):
        """_add_labels for (user row, item row) pairs (-1 = unknown): int32."""
        return ops.profile_labels(user_rows, item_rows, self.last_item, offline=offline)

"""GPU DIN ranker: drop-in for src/rank/DIN.py's scoring path.

* ``encode_samples`` / ``DinEncoder`` (nrk/rank/encode.py) restate
  DINDataset.__getitem__ + collate_fn (DIN.py:289-520) without a per-row
  loop: the same int index tensors (0 = pad / unknown, class index + 1
  otherwise; LAST T history items, left aligned, prefix mask), the lookups
  gathered on the device for ``DINRanker.predict``.
* ``DINScorer`` holds a trained DINModel's state_dict in kernel layout and
  scores batches with the HIP kernels (nrk_din_forward).
* ``DINRanker`` (a ``BaseRanker``, rank/base.py:10-117) is the plugin
  RankPipeline drives (rank_pipeline.py:96-141): ``load()`` (DIN.py:529-558),
  ``load_model(load_dir)`` (:1328-1399), ``predict()`` (:1219-1283): every
  main_df row in order, batches of ``batch_size``, probabilities positional
  to main_df.  Like the reference, Dice uses the statistics of each batch, so
  a batch is the unit of work; a trailing batch of one row is NaN there (std
  of one sample) and is NaN here too.
* ``DINRanker.train`` / ``train_on_encoded`` / ``save_model`` train the model
  on the device (ops.din_train_grad + ops.din_adam_step) and write the
  reference's artifacts.
"""
from __future__ import annotations

import os
import pickle
from collections.abc import Mapping
from typing import Optional

import numpy as np
import torch

from .. import ops
from ..config import RankConfig
from .base import BaseRanker, load_pickle


from .encode import DinEncoder, iloc_columns  # noqa: F401  (re-exported)


def encode_samples(user_ids, item_ids, ctx_cols, user_profile_dict, item_features_dict,
                   user_history_dict, user_features, item_features, ctx_features,
                   label_encoders, seq_max_len):
    """DINDataset + collate_fn for a list of samples (host arrays).
    ``user_ids``/``item_ids`` and ``ctx_cols`` (feature -> raw values) as the
    reference reads them from main_df rows (see ``iloc_columns``)."""
    enc = DinEncoder(user_profile_dict, item_features_dict, user_history_dict, user_features,
                     item_features, ctx_features, label_encoders, seq_max_len)
    return enc.encode_host(user_ids, item_ids, ctx_cols)


class DINScorer:
    """Trained DINModel weights (state_dict) on the device, scored by the HIP
    kernels.  ``table_dtype='bf16'`` stores the embedding tables in bf16
    (fp32 arithmetic)."""

    def __init__(self, state_dict, user_features, item_features, ctx_features,
                 table_dtype: str = "fp32", device="cuda"):
        self.device = torch.device(device)
        self.params = ops.DinParams(state_dict, user_features, item_features, ctx_features,
                                    table_dtype=table_dtype, device=self.device)

    def forward(self, user, item, hist, ctx, mask, logits=False):
        """One batch (B >= 2) of int index arrays -> probs (B,) [, logits]."""
        d = self.device
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(d, dt).contiguous()  # noqa: E731
        return ops.din_forward(self.params, t(user, torch.int32), t(item, torch.int32),
                               t(hist, torch.int32), t(ctx, torch.int32), t(mask, torch.float32),
                               logits=logits)

    def predict(self, enc, batch_size):
        """All rows in order, reference batching (DIN.py:1245-1283).  With a
        batch size that is a multiple of 64 every batch is scored in one
        nrk_din_forward_segments call (each batch keeps its own Dice
        statistics); otherwise one call per batch.  ``enc`` holds numpy
        arrays or device tensors (DinEncoder.encode_device)."""
        n = enc["mask"].shape[0]
        if n >= 2 and (batch_size % 64 == 0 or n <= batch_size):
            d = self.device
            t = lambda a, dt: torch.as_tensor(a).to(d, dt).contiguous()  # noqa: E731
            p = ops.din_forward(self.params, t(enc["user"], torch.int32), t(enc["item"], torch.int32),
                                t(enc["hist"], torch.int32), t(enc["ctx"], torch.int32),
                                t(enc["mask"], torch.float32), batch_size=batch_size)
            return p.cpu().numpy()
        out = np.empty(n, np.float32)
        for s in range(0, n, batch_size):
            e = min(n, s + batch_size)
            if e - s == 1:
                out[s] = np.nan  # std over one sample is NaN in the reference too
                continue
            host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in enc.items()}
            p = self.forward(host["user"][s:e], host["item"][s:e], host["hist"][s:e],
                             host["ctx"][s:e], host["mask"][s:e])
            out[s:e] = p.cpu().numpy()
        return out


def _expected_state(uv, iv, cv, dim, mlp_hidden, activation="dice"):
    """key -> shape of DINModel(uv, iv, cv, dim, [36], mlp_hidden, activation)'s
    state_dict (DIN.py:133-212; ActivationUnit is built with its defaults,
    :188, so it is Dice under either activation; each Dice holds an unused
    ``alpha``, each nn.PReLU() of the final MLP its one slope ``weight``,
    :203-206)."""
    exp = {}
    for grp, vocab in (("user_profile_embedding_dict", uv), ("item_embedding_dict", iv),
                       ("context_embedding_dict", cv)):
        for f, v in vocab.items():
            exp[f"{grp}.{f}.weight"] = (v, dim)
    item_dim = len(iv) * dim
    exp.update({"activation_unit.mlp.0.weight": (36, 4 * item_dim), "activation_unit.mlp.0.bias": (36,),
                "activation_unit.mlp.1.alpha": (), "activation_unit.mlp.2.weight": (1, 36),
                "activation_unit.mlp.2.bias": (1,)})
    cur = (len(uv) + len(cv)) * dim + 2 * item_dim
    for n, unit in enumerate(mlp_hidden):
        exp[f"mlp.{2 * n}.weight"], exp[f"mlp.{2 * n}.bias"] = (unit, cur), (unit,)
        if activation == "prelu":
            exp[f"mlp.{2 * n + 1}.weight"] = (1,)
        else:
            exp[f"mlp.{2 * n + 1}.alpha"] = ()
        cur = unit
    exp[f"mlp.{2 * len(mlp_hidden)}.weight"], exp[f"mlp.{2 * len(mlp_hidden)}.bias"] = (1, cur), (1,)
    return exp


def _batched_bce(probs, labels, batch_size):
    """Mean over the batches of nn.BCELoss per batch (DIN.py:946-965), and the
    accuracy at 0.5 over all rows."""
    p, y = np.asarray(probs, np.float64), np.asarray(labels, np.float64)
    losses = []
    for s in range(0, len(p), batch_size):
        q, t = p[s:s + batch_size], y[s:s + batch_size]
        with np.errstate(divide="ignore"):
            losses.append(float(np.mean(-(t * np.maximum(np.log(q), -100) + (1 - t) * np.maximum(np.log1p(-q), -100)))))
    return float(np.mean(losses)), float(np.mean((p > 0.5) == (y > 0.5)))


def _validation_metrics(labels, probs):
    """DIN.py:1065-1128: AUC, log loss, accuracy, precision, recall, F1 at 0.5."""
    from sklearn import metrics as M

    y, p = np.asarray(labels).astype(int), np.asarray(probs, np.float64)
    ok = np.isfinite(p)
    y, p = y[ok], p[ok]
    pred = (p > 0.5).astype(int)
    two = len(np.unique(y)) > 1
    return {"auc_roc": float(M.roc_auc_score(y, p)) if two else float("nan"),
            "log_loss": float(M.log_loss(y, np.clip(p, 1e-15, 1 - 1e-15), labels=[0, 1])),
            "accuracy": float(M.accuracy_score(y, pred)),
            "precision": float(M.precision_score(y, pred, zero_division=0)),
            "recall": float(M.recall_score(y, pred, zero_division=0)),
            "f1_score": float(M.f1_score(y, pred, zero_division=0))}


class DINRanker(BaseRanker):
    """Ranker plugin: drop-in for src/rank/DIN.py's DINRanker on the serving
    path RankPipeline drives (rank_pipeline.py:96-141):
    ``DINRanker(config)`` -> ``load()`` -> ``load_model(load_dir)`` ->
    ``predict()`` (probabilities positional to ``main_df`` rows).

    * ``load`` (DIN.py:529-558) reads ``main_features.csv`` and the
      user-profile / item-feature / user-history / feature-list pickles from
      the ``RankConfig`` paths;
    * ``load_model(load_dir=None)`` (DIN.py:1328-1399) reads
      ``din_model_metadata.pkl`` and ``label_encoders.pkl``, re-fits the
      encoders and vocabularies from the loaded data exactly as the
      reference's ``_prepare_vocab_dicts`` does (:560-619, which overwrites
      the pickled encoders), then ``din_model.pth`` through
      ``torch.load(weights_only=True)`` -- checked like a strict
      ``load_state_dict`` -- into device weights for the HIP kernels;
    * ``predict`` (:1219-1283): every main_df row in order, Dice batches of
      ``config.batch_size``.
    * ``train`` (:703-1005) runs on the device: the fused step of
      csrc/din_train.hip and its Adam sweep (``train_on_encoded`` is the
      deterministic core), then ``save_model`` (:1285-1326).
    Alternate entry points for in-memory data: ``set_data(...)`` and
    ``load_model(state_dict)``."""

    def __init__(self, config: Optional[RankConfig] = None, device="cuda", table_dtype="fp32"):
        super().__init__(config or RankConfig())
        self.device = device
        self.table_dtype = table_dtype
        self.model = None  # DINScorer: the model's weights on the device
        self.trainer = None  # ops.DinTrainParams: parameters and Adam moments while training
        self.label_encoders = {}
        self.encoder = None
        self._tables = None

    @property
    def scorer(self):
        return self.model

    # ------------------------------------------------------------ data --
    def load(self):
        """DIN.py:529-558."""
        import pandas as pd

        self.main_df = pd.read_csv(self.config.main_features_path)
        self.user_profile_dict = load_pickle(self.config.user_profile_dict_path)
        self.item_features_dict = load_pickle(self.config.item_features_dict_path)
        self.user_history_dict = load_pickle(self.config.user_history_dict_path)
        feature_lists = load_pickle(self.config.feature_lists_path)
        self.user_profile_features = feature_lists["user_profile_features"]
        self.item_features = feature_lists["item_features"]
        self.context_features = feature_lists["context_features"]
        self.encoder, self._tables = None, None

    def set_data(self, main_df, user_profile_dict, item_features_dict, user_history_dict,
                 user_profile_features, item_features, context_features, label_encoders):
        """The structures ``load()`` reads, handed over in memory (with the
        encoders the model was trained with)."""
        self.main_df = main_df
        self.user_profile_dict = user_profile_dict
        self.item_features_dict = item_features_dict
        self.user_history_dict = user_history_dict
        self.user_profile_features = list(user_profile_features)
        self.item_features = list(item_features)
        self.context_features = list(context_features)
        self.label_encoders = label_encoders
        self.encoder = DinEncoder(user_profile_dict, item_features_dict, user_history_dict,
                                  self.user_profile_features, self.item_features, self.context_features,
                                  label_encoders, self.config.din_seq_max_len)
        self._tables = None
        return self

    def _prepare_vocab_dicts(self):
        """DIN.py:560-619: one LabelEncoder per feature fitted on the loaded
        data (user / item features on their raw values, context features on
        ``main_df[feat].fillna(0).astype(str)``), stored in
        ``self.label_encoders``; vocabulary = classes + 1."""
        from sklearn.preprocessing import LabelEncoder

        uv, iv, cv = {}, {}, {}
        for feats, dicts, vocab in ((self.user_profile_features, list(self.user_profile_dict.values()), uv),
                                    (self.item_features, list(self.item_features_dict.values()), iv)):
            for feat in feats:
                values = {d[feat] for d in dicts if feat in d}
                if values:
                    le = LabelEncoder()
                    le.fit(list(values))
                    self.label_encoders[feat] = le
                    vocab[feat] = len(le.classes_) + 1
        ctx = self.main_df[self.context_features].copy()
        for feat in self.context_features:
            if feat in ctx.columns:
                le = LabelEncoder()
                ctx[feat] = ctx[feat].fillna(0)
                le.fit(ctx[feat].astype(str))
                self.label_encoders[feat] = le
                cv[feat] = len(le.classes_) + 1
        return uv, iv, cv

    # ----------------------------------------------------------- model --
    @staticmethod
    def _check_model_config(activation, hidden):
        """The model family the kernels serve and train."""
        if activation not in ops.DIN_ACTIVATIONS:
            raise NotImplementedError(f"the DIN kernels implement din_activation 'dice' and 'prelu', "
                                      f"got {activation!r}")
        if not 1 <= len(hidden) <= ops.DIN_MAX_LAYERS or not all(1 <= int(u) <= 1024 for u in hidden):
            raise NotImplementedError(f"the DIN kernels implement 1 to {ops.DIN_MAX_LAYERS} MLP hidden layers of "
                                      f"width 1 to 1024, got din_mlp_hidden_units = {hidden}")

    def load_model(self, load_dir=None):
        """DIN.py:1328-1399 (``load_dir``: a directory, default
        ``config.save_path``), or a DINModel state_dict (alternate entry)."""
        if isinstance(load_dir, Mapping):
            self.model = DINScorer(load_dir, self.user_profile_features, self.item_features, self.context_features,
                                   table_dtype=self.table_dtype, device=self.device)
            return self
        load_dir = load_dir or self.config.save_path
        metadata_path = os.path.join(load_dir, "din_model_metadata.pkl")
        if not os.path.exists(metadata_path):
            raise FileNotFoundError(f"Model metadata not found at: {metadata_path}")
        metadata = load_pickle(metadata_path)
        self.user_profile_features = metadata["user_profile_features"]
        self.item_features = metadata["item_features"]
        self.context_features = metadata["context_features"]
        encoders_path = os.path.join(load_dir, "label_encoders.pkl")
        self.label_encoders = load_pickle(encoders_path) if os.path.exists(encoders_path) else {}
        uv, iv, cv = self._prepare_vocab_dicts()
        activation = metadata.get("din_activation", "dice")
        hidden = list(metadata.get("din_mlp_hidden_units", [200, 80]))
        self._check_model_config(activation, hidden)
        model_path = os.path.join(load_dir, "din_model.pth")
        if not os.path.exists(model_path):
            raise FileNotFoundError(f"Model weights not found at: {model_path}")
        sd = torch.load(model_path, map_location="cpu", weights_only=True)
        exp = _expected_state(uv, iv, cv, int(metadata["din_embedding_dim"]), hidden, activation)
        missing, unexpected = sorted(set(exp) - set(sd)), sorted(set(sd) - set(exp))
        bad = [k for k in exp if k in sd and tuple(sd[k].shape) != exp[k]]
        if missing or unexpected or bad:  # load_state_dict(strict=True) refuses these
            raise RuntimeError(f"Error(s) in loading state_dict for DINModel: missing {missing}, "
                               f"unexpected {unexpected}, size mismatch {bad}")
        self.model = DINScorer(sd, list(uv), list(iv), list(cv), table_dtype=self.table_dtype, device=self.device)
        self.encoder, self._tables = None, None
        return self

    # ----------------------------------------------------------- train --
    def _apply_negative_sampling(self, df, ratio=None, dataset_name="Dataset"):
        """DIN.py:621-701 with the same pandas calls and ``random_seed``: all
        positives, ``int(n_pos * ratio)`` sampled negatives, concatenated and
        shuffled (host ETL; row for row the reference's frame)."""
        import pandas as pd

        if "label" not in df.columns:
            return df
        pos, neg = df[df["label"] == 1], df[df["label"] == 0]
        ratio = ratio if ratio is not None else self.config.negative_positive_ratio
        if len(pos) == 0:
            return df
        target = int(len(pos) * ratio)
        if target >= len(neg):
            return df
        seed = self.config.random_seed
        np.random.seed(seed)
        sampled = neg.sample(n=target, random_state=seed)
        balanced = pd.concat([pos, sampled], ignore_index=True)
        return balanced.sample(frac=1, random_state=seed).reset_index(drop=True)

    def _init_state(self, uv, iv, cv):
        """DINModel's initial state_dict (DIN.py:133-212) under
        ``torch.manual_seed(config.random_seed)``: throw-away CPU modules of
        the model's shapes built in the model's construction order (the
        nn.Embedding tables of the three groups, the ActivationUnit's two
        nn.Linear, the MLP's nn.Linear), so the generator is consumed exactly as
        ``DINModel(...)`` consumes it; a Dice ``alpha`` holds its layer's width,
        as the reference's ``Dice(unit)`` leaves it (unused, never trained).
        Under ``din_activation="prelu"`` every hidden layer of the MLP holds an
        ``nn.PReLU()`` slope instead: 0.25, drawn from no random numbers."""
        import torch.nn as nn

        dim, hidden = self.config.din_embedding_dim, list(self.config.din_mlp_hidden_units)
        activation = self.config.din_activation
        torch.manual_seed(self.config.random_seed)
        sd = {}
        for grp, vocab in (("user_profile_embedding_dict", uv), ("item_embedding_dict", iv),
                           ("context_embedding_dict", cv)):
            for f, v in vocab.items():
                sd[f"{grp}.{f}.weight"] = nn.Embedding(v, dim).weight.detach()
        item_dim = len(iv) * dim
        units = [("activation_unit.mlp.0", 4 * item_dim, 36), ("activation_unit.mlp.2", 36, 1)]
        cur = (len(uv) + len(cv)) * dim + 2 * item_dim
        for n, unit in enumerate(hidden):
            units.append((f"mlp.{2 * n}", cur, unit))
            cur = unit
        units.append((f"mlp.{2 * len(hidden)}", cur, 1))
        for name, fan_in, out in units:
            lin = nn.Linear(fan_in, out)
            sd[name + ".weight"], sd[name + ".bias"] = lin.weight.detach(), lin.bias.detach()
        # Dice(unit) hands the layer width to ``alpha`` (DIN.py:72, :204): 36.0, then the MLP widths
        sd["activation_unit.mlp.1.alpha"] = torch.tensor(36.0, dtype=torch.float32)
        for n, unit in enumerate(hidden):
            if activation == "prelu":
                sd[f"mlp.{2 * n + 1}.weight"] = torch.full((1,), 0.25, dtype=torch.float32)
            else:
                sd[f"mlp.{2 * n + 1}.alpha"] = torch.tensor(float(unit), dtype=torch.float32)
        return {k: sd[k] for k in _expected_state(uv, iv, cv, dim, hidden, activation)}

    def train_on_encoded(self, enc, labels, batch_size, epochs, learning_rate, order=None, init_state=None):
        """The deterministic core of ``train``: Adam over ``epochs`` passes of
        the encoded samples (``DinEncoder.encode_device`` output, or host
        arrays) in batches of ``batch_size``, the last one short
        (``drop_last=False``); a trailing batch of one row is skipped with a
        warning (its Dice std is NaN in the reference).  ``order``: an
        explicit [epochs, n] permutation; by default a device
        ``torch.randperm`` per epoch seeded with ``random_seed + epoch`` (a
        uniform permutation, not the DataLoader's draws).  ``init_state``: a
        DINModel state_dict to start from (default: continue the current
        trainer).  Per-step losses stay on the device and are read once per
        epoch: returns them as a CPU tensor and appends
        ``(epoch_fraction, loss)`` to ``loss_history``."""
        import warnings

        dev = torch.device(self.device)
        if init_state is not None or getattr(self, "trainer", None) is None:
            if init_state is None:
                raise ValueError("train_on_encoded needs init_state for the first call")
            self.trainer = ops.DinTrainParams(init_state, self.user_profile_features, self.item_features,
                                              self.context_features, table_dtype=self.table_dtype, device=dev)
        p = self.trainer
        t = lambda a, dt: torch.as_tensor(a).to(dev, dt).contiguous()  # noqa: E731
        data = [t(enc["user"], torch.int32), t(enc["item"], torch.int32), t(enc["hist"], torch.int32),
                t(enc["ctx"], torch.int32), t(enc["mask"], torch.float32), t(labels, torch.float32)]
        n = data[0].shape[0]
        ops.din_train_check(p, data[0], data[1], data[2], data[3], data[5])
        bounds = [(s, min(n, s + batch_size)) for s in range(0, n, batch_size)]
        if bounds and bounds[-1][1] - bounds[-1][0] == 1:
            warnings.warn("DIN training: the trailing batch of one row is skipped (Dice's std of one sample is NaN)")
            bounds.pop()
        if not bounds:
            raise ValueError("DIN training needs at least one batch of two rows")
        if order is not None:
            order = torch.as_tensor(order).to(dev, torch.int64).reshape(epochs, n)
        if not hasattr(self, "loss_history"):
            self.loss_history = []
        grads = {}
        all_losses = []
        for epoch in range(epochs):
            if order is not None:
                perm = order[epoch]
            else:
                gen = torch.Generator(device=dev)
                gen.manual_seed(int(self.config.random_seed) + epoch)
                perm = torch.randperm(n, device=dev, generator=gen)
            shuffled = [x.index_select(0, perm).contiguous() for x in data]
            losses = torch.zeros(len(bounds), dtype=torch.float32, device=dev)
            for i, (s, e) in enumerate(bounds):
                g = grads.get(e - s)
                g = grads[e - s] = ops.din_train_grad(p, *[x[s:e] for x in shuffled], out=g, loss=losses[i:i + 1],
                                                     validate=False)
                ops.din_adam_step(p, g, lr=learning_rate)
            host = losses.cpu()  # the epoch's one read
            all_losses.append(host)
            self.loss_history += [(epoch + (i + 1) / len(bounds), float(v)) for i, v in enumerate(host)]
        self.model = None  # the scorer of the previous weights is stale
        return torch.cat(all_losses)

    def state_dict(self):
        """The trained parameters under DINModel.state_dict()'s keys and order."""
        if getattr(self, "trainer", None) is None:
            raise ValueError("No model to save. Train the model first.")
        return self.trainer.state_dict()

    def _scorer_from_trainer(self):
        self.model = DINScorer(self.trainer.state_dict(), self.user_profile_features, self.item_features,
                               self.context_features, table_dtype=self.table_dtype, device=self.device)
        return self.model

    def _encode_frame(self, df):
        cols = iloc_columns(df, ["user_id", "item_id"] + list(self.context_features))
        return self.encoder.encode_device(self._tables, cols["user_id"], cols["item_id"], cols)

    def train(self):
        """DIN.py:703-1005 without the plots and the JSON log: split on
        ``is_train`` / ``is_val`` (80 / 20 of the rows without them), negative
        sampling of both parts, ``_prepare_vocab_dicts``, the reference's
        initialisation (``_init_state``), ``config.epochs`` epochs of
        ``train_on_encoded``, after each the validation loss and accuracy
        from the inference kernels in Dice batches of ``batch_size``
        (``val_loss_history``), the final validation metrics
        (``final_metrics``), then ``label_encoders.pkl`` and ``save_model``."""
        cfg = self.config
        if getattr(self, "main_df", None) is None:
            self.load()
        df = self.main_df
        if "is_train" in df.columns and "is_val" in df.columns:
            train_data, val_data = df[df["is_train"] == True].copy(), df[df["is_val"] == True].copy()  # noqa: E712
        else:
            cut = int(len(df) * 0.8)
            train_data, val_data = df.iloc[:cut].copy(), df.iloc[cut:].copy()
        if cfg.enable_negative_sampling and "label" in train_data.columns:
            train_data = self._apply_negative_sampling(train_data, cfg.negative_positive_ratio, "Training Set")
        if cfg.enable_negative_sampling and "label" in val_data.columns and len(val_data) > 0:
            val_data = self._apply_negative_sampling(val_data, cfg.negative_positive_ratio, "Validation Set")
        uv, iv, cv = self._prepare_vocab_dicts()
        self._check_model_config(cfg.din_activation, list(cfg.din_mlp_hidden_units))
        self.user_profile_features, self.item_features, self.context_features = list(uv), list(iv), list(cv)
        self.encoder = DinEncoder(self.user_profile_dict, self.item_features_dict, self.user_history_dict,
                                  self.user_profile_features, self.item_features, self.context_features,
                                  self.label_encoders, cfg.din_seq_max_len)
        self._tables = self.encoder.device_tables(torch.device(self.device))
        enc = self._encode_frame(train_data)
        labels = train_data["label"].to_numpy(np.float32)
        val_enc = self._encode_frame(val_data) if len(val_data) > 0 else None
        val_labels = val_data["label"].to_numpy(np.float32) if len(val_data) > 0 else None
        self.loss_history, self.val_loss_history, self.final_metrics = [], [], None
        init = self._init_state(uv, iv, cv)
        val_probs = None
        for epoch in range(cfg.epochs):
            gen = torch.Generator(device=torch.device(self.device))
            gen.manual_seed(int(cfg.random_seed) + epoch)
            perm = torch.randperm(len(labels), device=torch.device(self.device), generator=gen)
            before = len(self.loss_history)
            self.train_on_encoded(enc, labels, cfg.batch_size, 1, cfg.learning_rate, order=perm.reshape(1, -1),
                                  init_state=init if epoch == 0 else None)
            n_b = len(self.loss_history) - before
            self.loss_history[before:] = [(epoch + (i + 1) / n_b, v) for i, (_, v) in
                                          enumerate(self.loss_history[before:])]
            if val_enc is not None:
                val_probs = self._scorer_from_trainer().predict(val_enc, cfg.batch_size)
                loss, acc = _batched_bce(val_probs, val_labels, cfg.batch_size)
                self.val_loss_history.append((epoch + 1, loss))
                print(f"Epoch [{epoch + 1}/{cfg.epochs}] completed: Train Loss: "
                      f"{np.mean([v for _, v in self.loss_history[before:]]):.4f}, Val Loss: {loss:.4f}, "
                      f"Val Acc: {100 * acc:.2f}%")
        self._scorer_from_trainer()
        if val_probs is not None:
            self.final_metrics = _validation_metrics(val_labels, val_probs)
        os.makedirs(cfg.save_path, exist_ok=True)
        with open(os.path.join(cfg.save_path, "label_encoders.pkl"), "wb") as f:
            pickle.dump(self.label_encoders, f)
        self.save_model()
        return self

    def save_model(self, save_dir=None):
        """DIN.py:1285-1326: ``din_model.pth`` (the state_dict, DINModel's keys
        and order), ``din_model_metadata.pkl`` and ``label_encoders.pkl`` in
        the reference's formats; this ``load_model`` and the reference's read
        them."""
        from collections import OrderedDict

        sd = self.state_dict()
        save_dir = save_dir or self.config.save_path
        os.makedirs(save_dir, exist_ok=True)
        torch.save(OrderedDict(sd), os.path.join(save_dir, "din_model.pth"))
        metadata = {"user_profile_features": self.user_profile_features, "item_features": self.item_features,
                    "context_features": self.context_features, "din_embedding_dim": self.config.din_embedding_dim,
                    "din_attention_hidden_units": self.config.din_attention_hidden_units,
                    "din_mlp_hidden_units": self.config.din_mlp_hidden_units,
                    "din_activation": self.config.din_activation, "din_seq_max_len": self.config.din_seq_max_len}
        for name, obj in (("din_model_metadata.pkl", metadata), ("label_encoders.pkl", self.label_encoders)):
            with open(os.path.join(save_dir, name), "wb") as f:
                pickle.dump(obj, f)

    # --------------------------------------------------------- predict --
    def predict(self):
        """DIN.py:1219-1283: probabilities [len(main_df)] float32."""
        if self.model is None and self.trainer is not None:
            self._scorer_from_trainer()
        if self.model is None:
            raise ValueError("Model is not trained yet. Please train the model before prediction.")
        if not getattr(self, "label_encoders", None):
            encoders_path = os.path.join(self.config.save_path, "label_encoders.pkl")
            if os.path.exists(encoders_path):
                self.label_encoders = load_pickle(encoders_path)
        if getattr(self, "main_df", None) is None:
            raise ValueError("load() or set_data() must be called before predict()")
        if self.encoder is None:
            # the encoded lookup tables, built once per data set (the
            # reference's _build_encoding_cache, DIN.py:330-342, plus the
            # per-user / per-item dict lookups of __getitem__ as table rows)
            self.encoder = DinEncoder(self.user_profile_dict, self.item_features_dict, self.user_history_dict,
                                      self.user_profile_features, self.item_features, self.context_features,
                                      self.label_encoders, self.config.din_seq_max_len)
            self._tables = None
        cols = iloc_columns(self.main_df, ["user_id", "item_id"] + list(self.context_features))
        if self._tables is None:
            self._tables = self.encoder.device_tables(self.model.device)
        enc = self.encoder.encode_device(self._tables, cols["user_id"], cols["item_id"], cols)
        return self.model.predict(enc, self.config.batch_size)

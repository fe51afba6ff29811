"""Generate tests/golden/din_train_small*.npz by executing the REFERENCE's
DINModel, DINDataset and collate_fn (src/rank/DIN.py), imported through
make_golden.import_reference, under nn.BCELoss and torch.optim.Adam as
DINRanker.train wires them (:865-913), and its _apply_negative_sampling
(:621-701) on a labelled frame.  Runs only where make_golden.py runs.

Usage:  python tests/golden/make_golden_din_train.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

T = 8
BATCHES = [64] * 6 + [37]


def gen():
    import pandas as pd
    import torch
    import torch.nn as nn
    from sklearn.preprocessing import LabelEncoder
    from src.rank.DIN import DINDataset, DINModel, DINRanker, collate_fn
    from src.utils.config import RankConfig

    UF, IF, CF = mg.USER_FEATS, mg.ITEM_FEATS, mg.CTX_FEATS
    rng = np.random.default_rng(37)
    n_users, n_items, n_rows = 80, 120, sum(BATCHES)
    users = [str(u) for u in range(1000, 1000 + n_users)]
    items = [str(i) for i in range(5000, 5000 + n_items)]
    upd = {u: {f: float(np.round(rng.random() * 2, 1)) for f in UF} for u in users[: n_users - 4]}
    ifd = {it: {f: int(rng.integers(0, 20)) for f in IF} for it in items[: n_items - 6]}
    uhd = {}
    for u in users[n_users // 4:]:  # a quarter of the users have no history
        uhd[u] = [items[int(x)] for x in rng.integers(0, n_items, int(rng.integers(1, 14)))]
    main = pd.DataFrame({"user_id": [int(users[x]) for x in rng.integers(0, n_users, n_rows)],
                         "item_id": [int(items[x]) for x in rng.integers(0, n_items, n_rows)],
                         "label": rng.integers(0, 2, n_rows)})
    for f in CF:  # string bins: main_df.iloc[i] is an object row and str(user_id) finds the dict keys
        main[f] = rng.integers(0, 9, n_rows).astype(str)
    enc = {}
    for f, d in [(f, upd) for f in UF] + [(f, ifd) for f in IF]:
        enc[f] = LabelEncoder().fit(list({p[f] for p in d.values()}))
    for f in CF:
        enc[f] = LabelEncoder().fit(main[f].fillna(0).astype(str))
    uv = {f: len(enc[f].classes_) + 1 for f in UF}
    iv = {f: len(enc[f].classes_) + 1 for f in IF}
    cv = {f: len(enc[f].classes_) + 1 for f in CF}
    assert max(list(uv.values()) + list(iv.values()) + list(cv.values())) <= 24

    ds = DINDataset(main, upd, ifd, uhd, UF, IF, CF, "label", enc)
    torch.set_num_threads(1)
    mg.seed_all(23)
    model = DINModel(uv, iv, cv, embedding_dim=32, attention_hidden_units=[36], mlp_hidden_units=[200, 80],
                     activation="dice")
    model.train()
    init = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = nn.BCELoss()
    losses, grads, start, enc_batches = [], {}, 0, []
    for step, bs in enumerate(BATCHES):
        batch = collate_fn([ds[i] for i in range(start, start + bs)], seq_max_len=T)
        start += bs
        enc_batches.append(batch)
        opt.zero_grad()
        loss = crit(model(batch), batch["labels"])
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        losses.append(loss.item())
    final = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    cat = lambda grp, feats, ax: np.concatenate(  # noqa: E731
        [np.stack([b[grp][f].numpy() for f in feats], ax) for b in enc_batches], 0)
    mask = np.concatenate([b["history_mask"].numpy() for b in enc_batches], 0)
    arrays = dict(
        user_features=np.array(UF), item_features=np.array(IF), context_features=np.array(CF),
        user=cat("user_profile", UF, 1), item=cat("recall_item", IF, 1), hist=cat("history_items", IF, 2),
        ctx=cat("context", CF, 1), mask=mask.astype(np.float32),
        label=np.concatenate([b["labels"].numpy() for b in enc_batches], 0).astype(np.float32),
        batch_sizes=np.array(BATCHES, np.int64), losses=np.array(losses, np.float64), lr=np.float64(1e-3),
        seq_max_len=np.int64(T),
    )
    for k in init:
        arrays["init." + k] = init[k]
        arrays["final." + k] = final[k]
    for k in grads:
        arrays["grad." + k] = grads[k]

    # _apply_negative_sampling on a 1:14 frame: the kept rows, by their position in the input
    import tempfile

    n = 3000
    frame = pd.DataFrame({"row": np.arange(n), "label": (rng.random(n) < 1 / 15).astype(np.int64)})
    with tempfile.TemporaryDirectory() as tmp:
        ranker = DINRanker(RankConfig(_project_root=tmp))
        arrays["ns_seed"] = np.int64(ranker.config.random_seed)
        arrays["ns_ratio"] = np.float64(4.0)
        sampled = ranker._apply_negative_sampling(frame, ratio=4.0, dataset_name="fixture")
    arrays["ns_label"] = frame["label"].to_numpy(np.int64)
    arrays["ns_rows"] = sampled["row"].to_numpy(np.int64)
    out = mg.save_parts(os.path.join(HERE, "din_train_small.npz"), **arrays)
    print(f"din_train_small: {n_rows} rows, {int((mask.sum(1) == 0).sum())} without history, vocab <= "
          f"{max(list(uv.values()) + list(iv.values()) + list(cv.values()))}, losses {losses[0]:.6f} .. "
          f"{losses[-1]:.6f}, negative sampling keeps {len(sampled)} of {n} -> {[os.path.basename(p) for p in out]}")


def main():
    mg.import_reference()
    gen()


if __name__ == "__main__":
    main()

"""Generate tests/golden/ytdnn_train_small*.npz by executing the REFERENCE's
YoutubeDNNRecaller._prepare_data, collate_fn and YoutubeDNN module
(youtubednn_recaller.py), imported through make_golden.import_reference, under
torch.optim.Adam and BCEWithLogitsLoss as YoutubeDNNRecaller.train wires them
(:381-412).  Runs only where make_golden.py runs.

Usage:  python tests/golden/make_golden_ytdnn_train.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

T, DIM, HIDDEN = 30, 16, [64, 16]
BATCHES = [64] * 6 + [37]


def gen():
    import pandas as pd
    import torch
    import torch.nn as nn
    from nrk.data import synth
    from sklearn.preprocessing import LabelEncoder
    from src.recall.youtubednn_recaller import YoutubeDNN, YoutubeDNNRecaller, collate_fn
    from src.utils.config import RecallConfig

    log = synth.make_click_log(n_users=300, n_items=500, seed=5, max_len=40)
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(log.user_id))  # click_df row order != time order
    click_df = pd.DataFrame({"user_id": log.user_id[perm] * 3 + 100,
                             "click_article_id": log.click_article_id[perm] * 7 + 11,
                             "click_timestamp": log.click_timestamp[perm]})
    # label encoding as train() does (:331-337)
    click_df["user_id"] = LabelEncoder().fit_transform(click_df["user_id"])
    click_df["click_article_id"] = LabelEncoder().fit_transform(click_df["click_article_id"])
    n_users = int(click_df["user_id"].max()) + 1
    n_items = int(click_df["click_article_id"].max()) + 1

    mg.seed_all(23)
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        rec = YoutubeDNNRecaller(RecallConfig(_project_root=tmp))
        train_set, _ = rec._prepare_data(click_df, negsample=0)
    triples = np.array(sorted((int(u), int(n), int(t)) for u, _, t, _, n in train_set), np.int64)
    assert all(len(h) == n for _, h, _, _, n in train_set)

    # fixed batches: a few samples with pos > T first, so truncation is on the path
    long_ = [s for s in train_set if s[4] > T][:8]
    assert long_, "no position beyond seq_max_len"
    rest = [s for s in train_set if s[4] <= T]
    chosen = (long_ + rest)[:sum(BATCHES)]
    order = rng.permutation(len(chosen))
    chosen = [chosen[i] for i in order]
    # mixed labels: every third sample becomes a negative with a random target
    samples = []
    for n, (u, h, t, lab, hl) in enumerate(chosen):
        if n % 3 == 1:
            t, lab = int(rng.integers(0, n_items)), 0
        samples.append((int(u), [int(x) for x in h], int(t), int(lab), int(hl)))

    torch.manual_seed(23)
    torch.set_num_threads(1)
    model = YoutubeDNN(n_users, n_items, DIM, HIDDEN)
    for m in model.modules():
        if isinstance(m, nn.Dropout):
            m.p = 0.0
    model.train()
    init = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = nn.BCEWithLogitsLoss()
    losses, grads, start = [], {}, 0
    for step, bs in enumerate(BATCHES):
        rows = [dict(user_id=u, hist_items=h, target_item=t, hist_len=hl, label=lab)
                for u, h, t, lab, hl in samples[start:start + bs]]
        start += bs
        batch = collate_fn(rows, seq_max_len=T)
        opt.zero_grad()
        ue, ie = model(batch["user_id"], batch["hist_items"], batch["hist_len"], batch["target_item"])
        loss = crit((ue * ie).sum(dim=1), batch["label"])
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters()}
        opt.step()
        losses.append(loss.item())
    final = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}

    arrays = dict(
        click_user=click_df["user_id"].to_numpy(np.int64),
        click_item=click_df["click_article_id"].to_numpy(np.int64),
        click_ts=click_df["click_timestamp"].to_numpy(np.int64),
        s_user=np.array([s[0] for s in samples], np.int64), s_pos=np.array([s[4] for s in samples], np.int64),
        s_target=np.array([s[2] for s in samples], np.int64), s_label=np.array([s[3] for s in samples], np.float32),
        batch_sizes=np.array(BATCHES, np.int64), losses=np.array(losses, np.float64), positives=triples,
        seq_max_len=np.int64(T), dim=np.int64(DIM), hidden=np.array(HIDDEN, np.int64), lr=np.float64(1e-3),
    )
    for k in init:
        arrays["init." + k] = init[k]
        arrays["grad." + k] = grads[k]
        arrays["final." + k] = final[k]
    out = mg.save_parts(os.path.join(HERE, "ytdnn_train_small.npz"), **arrays)
    print(f"ytdnn_train_small: {n_users} users, {n_items} items, {len(train_set)} positives, "
          f"{sum(s[4] > T for s in samples)} samples beyond T, {int(sum(s[3] for s in samples))} label-1 of "
          f"{len(samples)}, losses {losses[0]:.6f} .. {losses[-1]:.6f} -> {[os.path.basename(p) for p in out]}")


def main():
    mg.import_reference()
    gen()


if __name__ == "__main__":
    main()

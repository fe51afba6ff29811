"""Generate tests/golden/din_train_layers_small*.npz by executing the
REFERENCE's DINModel (src/rank/DIN.py), imported through
make_golden.import_reference, in train mode under nn.BCELoss and
torch.optim.Adam exactly as make_golden_din_train.py does, for models of other
depths and with the PReLU activation: the data set, 7 batches (6 x 64 + 37)
and learning rate are din_train_small's, and so is the seed wherever the run
stays clear of PReLU's kink (min |z| >= 16 e_z at every PReLU and step;
otherwise the next seed that does, stored per model).  The encoded index
tensors are asserted equal to din_train_small's and not stored again; of the
initial state only what differs from din_train_small's init.* is stored --
under its seed that is the MLP alone, since DINModel draws the embedding
tables and the attention unit before it.  Runs only where make_golden.py runs.

Usage:  python tests/golden/make_golden_din_train_layers.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

T = 8
BATCHES = [64] * 6 + [37]
SEED = 23  # din_train_small's: the tables and the attention unit are its init.*
MAX_SEEDS = 32
KINK = 16.0  # min |z| >= KINK * e_z at every PReLU, every step (tests/test_din_train_layers_host.py)


def dataset():
    """din_train_small's data set (make_golden_din_train.gen, the same draws)."""
    import pandas as pd
    from sklearn.preprocessing import LabelEncoder
    from src.rank.DIN import DINDataset

    UF, IF, CF = mg.USER_FEATS, mg.ITEM_FEATS, mg.CTX_FEATS
    rng = np.random.default_rng(37)
    n_users, n_items, n_rows = 80, 120, sum(BATCHES)
    users = [str(u) for u in range(1000, 1000 + n_users)]
    items = [str(i) for i in range(5000, 5000 + n_items)]
    upd = {u: {f: float(np.round(rng.random() * 2, 1)) for f in UF} for u in users[: n_users - 4]}
    ifd = {it: {f: int(rng.integers(0, 20)) for f in IF} for it in items[: n_items - 6]}
    uhd = {}
    for u in users[n_users // 4:]:
        uhd[u] = [items[int(x)] for x in rng.integers(0, n_items, int(rng.integers(1, 14)))]
    main = pd.DataFrame({"user_id": [int(users[x]) for x in rng.integers(0, n_users, n_rows)],
                         "item_id": [int(items[x]) for x in rng.integers(0, n_items, n_rows)],
                         "label": rng.integers(0, 2, n_rows)})
    for f in CF:
        main[f] = rng.integers(0, 9, n_rows).astype(str)
    enc = {}
    for f, d in [(f, upd) for f in UF] + [(f, ifd) for f in IF]:
        enc[f] = LabelEncoder().fit(list({p[f] for p in d.values()}))
    for f in CF:
        enc[f] = LabelEncoder().fit(main[f].fillna(0).astype(str))
    vocabs = tuple({f: len(enc[f].classes_) + 1 for f in feats} for feats in (UF, IF, CF))
    return DINDataset(main, upd, ifd, uhd, UF, IF, CF, "label", enc), vocabs


def train_model(name, hidden, act, seed, vocabs, feats, enc_batches, np_batches):
    """The reference's 7 steps under ``seed``: (init, final, step-1 gradients,
    losses, smallest prelu_gap), or None where a PReLU model misses the kink
    condition at some step."""
    import torch
    import torch.nn as nn
    from src.rank.DIN import DINModel

    import din_train_layers_restated as RL

    mg.seed_all(seed)
    model = DINModel(*vocabs, embedding_dim=32, attention_hidden_units=[36], mlp_hidden_units=list(hidden),
                     activation=act)
    model.train()
    init = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    assert list(init) == RL.state_keys(feats, len(hidden), act)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = nn.BCELoss()
    losses, grads, gaps = [], {}, []
    for step, batch in enumerate(enc_batches):
        if act == "prelu":
            now = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
            gaps.append(RL.prelu_gap(now, feats, np_batches[step]))
        opt.zero_grad()
        loss = crit(model(batch), batch["labels"])
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
        opt.step()
        losses.append(loss.item())
    final = {k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    gap = None
    if act == "prelu":
        gap = min(gaps, key=lambda g: g[0] / g[1])
        print(f"{name} seed {seed}: smallest PReLU gap over the 7 steps: min |z| {gap[0]:.3e}, e_z {gap[1]:.3e}, "
              f"ratio {gap[0] / gap[1]:.1f}")
        if not gap[0] >= KINK * gap[1]:
            return None
    return init, final, grads, losses, gap


def gen():
    import torch
    from src.rank.DIN import collate_fn

    import din_train_layers_restated as RL

    UF, IF, CF = mg.USER_FEATS, mg.ITEM_FEATS, mg.CTX_FEATS
    feats = (UF, IF, CF)
    ds, (uv, iv, cv) = dataset()
    small = {}
    for path in sorted(os.listdir(HERE)):
        if path.startswith("din_train_small.") and path.endswith(".npz"):
            with np.load(os.path.join(HERE, path)) as z:
                small.update({k: z[k] for k in z.files})
    torch.set_num_threads(1)
    start, enc_batches = 0, []
    for bs in BATCHES:
        enc_batches.append(collate_fn([ds[i] for i in range(start, start + bs)], seq_max_len=T))
        start += bs
    cat = lambda grp, fs, ax: np.concatenate(  # noqa: E731
        [np.stack([b[grp][f].numpy() for f in fs], ax) for b in enc_batches], 0)
    data = dict(user=cat("user_profile", UF, 1), item=cat("recall_item", IF, 1), hist=cat("history_items", IF, 2),
                ctx=cat("context", CF, 1),
                mask=np.concatenate([b["history_mask"].numpy() for b in enc_batches], 0).astype(np.float32),
                label=np.concatenate([b["labels"].numpy() for b in enc_batches], 0).astype(np.float32))
    for k, v in data.items():
        assert np.array_equal(v, small[k]), f"{k}: not din_train_small's"
    bounds = np.concatenate([[0], np.cumsum(BATCHES)])
    np_batches = [{k: v[a:b] for k, v in data.items()} for a, b in zip(bounds[:-1], bounds[1:])]

    arrays = dict(models=np.array(list(RL.MODELS)), lr=np.float64(1e-3))
    for name, (hidden, act) in RL.MODELS.items():
        # din_train_small's seed first: the tables and the attention unit are then its init.*; a PReLU
        # model whose run comes within rounding of a kink under that seed takes the next one that does not
        for seed in range(SEED, SEED + MAX_SEEDS):
            run = train_model(name, hidden, act, seed, (uv, iv, cv), feats, enc_batches, np_batches)
            if run is not None:
                break
        else:
            raise AssertionError(f"{name}: no seed in [{SEED}, {SEED + MAX_SEEDS}) meets the kink condition")
        init, final, grads, losses, gap = run
        arrays[f"{name}.seed"] = np.int64(seed)
        stored = 0
        for k in init:  # only what din_train_small does not hold already
            if k.startswith("mlp.") or not np.array_equal(init[k], small["init." + k]):
                arrays[f"{name}.init.{k}"] = init[k]
                stored += 1
        assert seed != SEED or stored == sum(k.startswith("mlp.") for k in init), "seed 23 draws din_train_small's init"
        for k in final:
            arrays[f"{name}.final.{k}"] = final[k]
        for k in grads:
            arrays[f"{name}.grad.{k}"] = grads[k]
        arrays[f"{name}.losses"] = np.array(losses, np.float64)
        if gap is not None:
            arrays[f"{name}.prelu_gap"] = np.array(gap, np.float64)
        print(f"{name}: seed {seed}, losses {losses[0]:.6f} .. {losses[-1]:.6f}")
    out = mg.save_parts(os.path.join(HERE, "din_train_layers_small.npz"), **arrays)
    print([os.path.basename(p) for p in out])


def main():
    mg.import_reference()
    gen()


if __name__ == "__main__":
    main()

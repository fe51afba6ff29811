"""Generate tests/golden/din_layers_small.npz by executing the REFERENCE's
DINModel (src/rank/DIN.py:133-286) in eval mode on the CPU, as its own
DINRanker.load / load_model / predict drive it (:529-558, :1328-1399,
:1219-1283), for three final-MLP configurations nrk did not serve before:

    prelu_24x10    din_activation "prelu", din_mlp_hidden_units [24, 10]
    dice_24x10x2   "dice", [24, 10, 2] (the shape of DINModel's own default)
    prelu_12       "prelu", [12]

The reference is imported through make_golden.import_reference; the artifacts
(main frame, profile / item-feature / history dicts) are make_golden's
rank_pipeline_data, so vocabularies stay below 70 rows per feature at embedding
width 32.  nn.PReLU() initialises every slope to 0.25; the slopes are set to
distinct values (one above 1, one negative) before the model is saved, as a
trained checkpoint would have them.  Stored: the artifacts, the index tensors
the reference's collate_fn handed to the model (shared by the three models),
the embedding tables and attention unit (copied into all three models, so
"front::sd::" holds them once), and per model the final MLP's state_dict
entries, the probabilities predict() returned and the logits in front of the
sigmoid.  The file is about 390 KB: most of it is the artifacts the
plugin-level test loads through DINRanker.load (400 rows, 70 users, 160 items,
25 features at width 32) and the 36 x 512 attention weights; the three MLPs
themselves are a few KB each.  Runs only where make_golden.py runs.

Usage:  python tests/golden/make_golden_din_layers.py
"""
from __future__ import annotations

import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

MODELS = [("prelu_24x10", "prelu", [24, 10], [1.5, -0.3]),
          ("dice_24x10x2", "dice", [24, 10, 2], None),
          ("prelu_12", "prelu", [12], [0.4])]
BATCH = 128  # DINRanker.predict's batch_size: 400 rows -> Dice batches of 128, 128, 128, 16


def gen(tmp):
    import torch
    from src.rank.DIN import DINModel, DINRanker
    from src.utils.config import RankConfig

    torch.set_num_threads(1)
    UF, IF, CF = mg.USER_FEATS, mg.ITEM_FEATS, mg.CTX_FEATS
    main, upd, ifd, uhd, lists = mg.rank_pipeline_data(53)
    out = {"main": main[["user_id", "item_id"] + CF + ["label"]].to_numpy(np.int64),
           "prof_users": np.array(list(upd), dtype=str),
           "prof_vals": np.array([[upd[u][f] for f in UF] for u in upd], np.float64),
           "ifeat_items": np.array(list(ifd), dtype=str),
           "ifeat_vals": np.array([[ifd[i][f] for f in IF] for i in ifd], np.int64),
           "hist_users": np.array(list(uhd), dtype=str),
           "hist_offsets": np.cumsum([0] + [len(v) for v in uhd.values()]).astype(np.int64),
           "hist_items": np.array([i for v in uhd.values() for i in v], dtype=str),
           "user_feats": np.array(UF), "item_feats": np.array(IF), "ctx_feats": np.array(CF),
           "batch_size": np.int64(BATCH), "models": np.array([m[0] for m in MODELS])}
    for n, (tag, act, hidden, slopes) in enumerate(MODELS):
        root = os.path.join(tmp, tag)
        cfg = RankConfig(_project_root=root, din_embedding_dim=32, din_mlp_hidden_units=hidden, din_activation=act,
                         batch_size=BATCH, num_workers=0, pin_memory=False)
        mg.write_rank_artifacts(cfg.save_path, main, upd, ifd, uhd, lists)
        r0 = DINRanker(cfg)
        r0.load()
        uv, iv, cv = r0._prepare_vocab_dicts()
        mg.seed_all(61 + n)
        r0.model = DINModel(uv, iv, cv, embedding_dim=32, attention_hidden_units=[36], mlp_hidden_units=hidden,
                            activation=act)
        with torch.no_grad():
            r0.model.activation_unit.mlp[0].weight.mul_(4.0)  # spread the attention weights (gen_rank_pipeline)
            for lin in [m for m in r0.model.mlp if isinstance(m, torch.nn.Linear)]:
                lin.weight.mul_(2.0)  # and the logits
            if n == 0:
                front = {k: v.clone() for k, v in r0.model.state_dict().items() if not k.startswith("mlp.")}
            else:  # one set of tables and one attention unit for the three models: stored once
                r0.model.load_state_dict(front, strict=False)
            if slopes:
                for k, a in enumerate(slopes):
                    r0.model.mlp[2 * k + 1].weight.fill_(a)
        r0.save_model(cfg.save_path)
        with open(os.path.join(cfg.save_path, "label_encoders.pkl"), "wb") as f:
            pickle.dump(r0.label_encoders, f)
        # the reference's serving path: load, load_model (rebuilds DINModel from the metadata), predict
        r = DINRanker(RankConfig(_project_root=root, din_embedding_dim=32, din_mlp_hidden_units=hidden,
                                 din_activation=act, batch_size=BATCH, num_workers=0, pin_memory=False))
        r.load()
        r.load_model(load_dir=cfg.save_path)
        batches, logits = [], []
        r.model.register_forward_pre_hook(lambda m, a: batches.append(a[0]))
        r.model.mlp.register_forward_hook(lambda m, i, o: logits.append(o.detach().cpu().numpy()[:, 0]))
        probs = r.predict().astype(np.float32)
        assert not r.model.training
        sd = torch.load(os.path.join(cfg.save_path, "din_model.pth"), weights_only=True)
        assert sorted(sd) == sorted(r.model.state_dict())
        for k, v in sd.items():  # "front::sd::" keys belong to every model's state_dict
            if k.startswith("mlp."):
                out[f"{tag}::sd::{k}"] = v.numpy()
            elif n == 0:
                out[f"front::sd::{k}"] = v.numpy()
            else:
                assert np.array_equal(out[f"front::sd::{k}"], v.numpy()), k
        out[f"{tag}::probs"] = probs
        out[f"{tag}::logits"] = np.concatenate(logits).astype(np.float32)
        out[f"{tag}::hidden"] = np.array(hidden, np.int64)
        out[f"{tag}::activation"] = np.array(act)
        cat = lambda grp, feats: np.concatenate(  # noqa: E731
            [np.stack([b[grp][f].cpu().numpy() for f in feats], -1) for b in batches], 0)
        inputs = {"user": cat("user_profile", UF).astype(np.int16), "item": cat("recall_item", IF).astype(np.int16),
                  "hist": cat("history_items", IF).astype(np.int16), "ctx": cat("context", CF).astype(np.int16),
                  "mask": np.concatenate([b["history_mask"].cpu().numpy() for b in batches], 0).astype(np.uint8)}
        for k, v in inputs.items():
            if n == 0:
                out[k] = v
            else:
                assert np.array_equal(out[k], v), k  # the encoding does not depend on the model
        if n == 0:
            for f, le in r0.label_encoders.items():
                c = np.asarray(le.classes_)
                out[f"classes::{f}"] = c.astype(str) if c.dtype == object else c
        lg = out[f"{tag}::logits"]
        print(f"{tag}: {len(probs)} rows, logits std {lg.std():.3f}, max |logit| {np.abs(lg).max():.2f}")
    paths = mg.save_parts(os.path.join(HERE, "din_layers_small.npz"), **out)
    print("din_layers_small:", [(os.path.basename(p), os.path.getsize(p)) for p in paths])


if __name__ == "__main__":
    mg.import_reference()
    with tempfile.TemporaryDirectory() as tmp:
        gen(tmp)

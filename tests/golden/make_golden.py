"""Generate the golden fixtures under tests/golden/ by importing the REFERENCE.

Runs only in the build container (it reads /root/reference, which does not
exist on the GPU box).  The reference is pure Python; it is imported with two
shims documented in SURVEY.md §8c:

* ``faiss`` is not installed (pyproject.toml:21 pins faiss-cpu>=1.7.4, not
  vendored).  A stand-in module provides ``IndexFlatIP`` restating the Faiss
  contract: exact inner product (fp64, products accumulated sequentially over
  the dimension), results sorted by score desc, ties -> lower row, labels -1 /
  scores -FLT_MAX when k > ntotal.  Parity at that boundary is therefore
  pinned to the restated contract, not to a Faiss binary.
* ``RecallConfig`` / ``RankConfig`` get ``_project_root=<tmp>`` because their
  ``__post_init__`` makes directories (config.py:60-71).

Everything else -- ItemCFSimilarity.calculate, ItemCFRecaller.recall,
YoutubeDNN / YoutubeDNNRecaller.train/_extract_embeddings/recall, DINModel,
DINDataset, collate_fn -- is the reference's own code, executed unchanged.

Usage:  python tests/golden/make_golden.py   (writes *.npz next to this file)

No committed file may exceed 1 MiB, so a fixture that would is written as
parts (save_parts: <name>.0.npz, <name>.1.npz, ...), which the ``golden``
fixture of tests/conftest.py puts together again, array for array.
"""
from __future__ import annotations

import os
import random
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "news-recommendation-tc_amd"))
REF = "/root/reference"

FLT_MAX = np.float32(3.4028234663852886e38)


class IndexFlatIP:
    """Stand-in for faiss.IndexFlatIP (the contract, restated)."""

    def __init__(self, d):
        self.d = int(d)
        self.xb = np.zeros((0, self.d), dtype=np.float32)

    @property
    def ntotal(self):
        return self.xb.shape[0]

    def add(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.xb = np.concatenate([self.xb, x], 0)

    def search(self, q, k):
        q = np.ascontiguousarray(q, dtype=np.float32)
        nq, n = q.shape[0], self.ntotal
        D = np.full((nq, k), -FLT_MAX, dtype=np.float32)
        I = np.full((nq, k), -1, dtype=np.int64)
        xb64 = self.xb.astype(np.float64)
        rows = np.arange(n)
        for qi in range(nq):
            s = np.zeros(n, dtype=np.float64)
            for t in range(self.d):  # sequential accumulation over the dimension
                s = s + np.float64(q[qi, t]) * xb64[:, t]
            order = np.lexsort((rows, -s))[: min(k, n)]
            D[qi, : len(order)] = s[order].astype(np.float32)
            I[qi, : len(order)] = order
        return D, I


PART_BYTES = 800_000  # compressed bytes per part, well under the 1 MiB limit for a committed file


def save_parts(path, **arrays):
    """np.savez_compressed(path, **arrays) while the file stays under 1 MiB;
    else parts of at most PART_BYTES, <name>.0.npz, <name>.1.npz, ...: "__keys__" in part 0
    holds the keys in order, every part holds whole arrays, and an array too
    large for one part is cut along axis 0 into pieces "<key>@@<i>of<n>" (the
    loader concatenates them).  Lossless: same keys, order, dtypes, values."""
    import io
    import zlib

    stem = path[:-len(".npz")]
    for old in os.listdir(HERE):  # the other form of the same fixture
        if old == os.path.basename(path) or (old.startswith(os.path.basename(stem) + ".") and old.endswith(".npz")):
            os.remove(os.path.join(HERE, old))
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    if buf.tell() < 1 << 20:
        with open(path, "wb") as fh:
            fh.write(buf.getvalue())
        return [path]
    assert "__keys__" not in arrays and not any("@@" in k for k in arrays)
    size = lambda a: len(zlib.compress(np.ascontiguousarray(a).tobytes(), 6)) + 512  # noqa: E731
    items = []
    for k, a in arrays.items():
        n = -(-size(a) // (PART_BYTES // 2))  # pieces no larger than half a part
        if n == 1 or a.ndim == 0:
            items.append((k, a))
        else:
            items += [(f"{k}@@{i}of{n}", piece) for i, piece in enumerate(np.array_split(a, n, axis=0))]
    parts, used = [{"__keys__": np.array(list(arrays))}], size(np.array(list(arrays)))
    for k, a in items:
        if used + size(a) > PART_BYTES:
            parts.append({})
            used = 0
        parts[-1][k] = a
        used += size(a)
    out = []
    for i, part in enumerate(parts):
        out.append(f"{stem}.{i}.npz")
        np.savez_compressed(out[-1], **part)
        assert os.path.getsize(out[-1]) < 1 << 20, out[-1]
    return out


def import_reference():
    sys.dont_write_bytecode = True
    if REF not in sys.path:
        sys.path.insert(0, REF)
    fa = types.ModuleType("faiss")
    fa.IndexFlatIP = IndexFlatIP
    sys.modules["faiss"] = fa
    import src.utils.config as cfg  # noqa: F401

    return cfg


def seed_all(s=23):
    import torch

    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


# --------------------------------------------------------------------------
# ItemCF (item_cf.py:17-89, itemcf_recaller.py:41-129)
# --------------------------------------------------------------------------
def gen_itemcf(tmp):
    import pandas as pd
    from nrk.data import synth
    from src.utils.config import RecallConfig
    from src.similarity.item_cf import ItemCFSimilarity
    from src.recall.itemcf_recaller import ItemCFRecaller
    from src.data.extractors import ItemFeatureExtractor, UserFeatureExtractor

    n_users, n_items = 2000, 5000
    log = synth.make_click_log(n_users=n_users, n_items=n_items, seed=7)
    art = synth.make_articles(n_items, seed=7)
    # raw ids that are not 0..n-1 so id handling is exercised
    click_df = pd.DataFrame(
        {
            "user_id": log.user_id * 3 + 100,
            "click_article_id": log.click_article_id * 7 + 11,
            "click_timestamp": log.click_timestamp,
        }
    )
    articles_df = pd.DataFrame(
        {
            "click_article_id": art.article_id * 7 + 11,
            "category_id": art.category_id,
            "words_count": art.words_count,
            "created_at_ts": art.created_at_ts,
        }
    )
    _, _, created = ItemFeatureExtractor.get_item_info_dict(articles_df)
    hot = ItemFeatureExtractor.get_item_topk_click(click_df, k=50)
    uit = UserFeatureExtractor.get_user_item_time_dict(click_df)

    cfg = RecallConfig(_project_root=tmp)
    sim = ItemCFSimilarity(cfg).calculate(click_df, created)

    rows_i, si, sj, sv = [], [], [], []
    for i, d in sim.items():
        rows_i.append(i)
        for j, v in d.items():
            si.append(i)
            sj.append(j)
            sv.append(v)
    cfg30 = RecallConfig(_project_root=tmp)
    rec = ItemCFRecaller(cfg30, sim, created, uit, hot, emb_similarity_matrix={})
    users = list(uit.keys()) + [-5, -6, 10**9]  # three unknown users (cold start)
    res = rec.batch_recall(users, topk=30)
    ru, ri, rs, roff = [], [], [], [0]
    for u in users:
        for it, sc in res[u]:
            ri.append(it)
            rs.append(sc)
        ru.append(u)
        roff.append(len(ri))
    # the same recall with the content weight of EmbeddingSimilarity (itemcf_recaller.py:98-103)
    from src.similarity.embedding import EmbeddingSimilarity

    erng = np.random.default_rng(17)
    art_ids = articles_df["click_article_id"].to_numpy(np.int64)
    eemb = erng.standard_normal((len(art_ids), 16)).astype(np.float32)
    edf = pd.DataFrame(eemb, columns=[f"emb_{n}" for n in range(16)])
    edf.insert(0, "article_id", art_ids)
    esim = EmbeddingSimilarity(RecallConfig(_project_root=tmp)).calculate(edf)
    ei, ej, ev = [], [], []
    for a, dd in esim.items():
        for b, v in dd.items():
            ei.append(a)
            ej.append(b)
            ev.append(v)
    erec = ItemCFRecaller(RecallConfig(_project_root=tmp), sim, created, uit, hot, emb_similarity_matrix=esim)
    eres = erec.batch_recall(users, topk=30)
    eri, ers, eroff = [], [], [0]
    for u in users:
        for it, sc in eres[u]:
            eri.append(it)
            ers.append(sc)
        eroff.append(len(eri))
    # user_item_time_dict as CSR (checks the host-side list builder)
    uu, uoff, uitems, uts = [], [0], [], []
    for u, lst in uit.items():
        uu.append(u)
        for it, ts in lst:
            uitems.append(it)
            uts.append(ts)
        uoff.append(len(uitems))
    cids = np.array(sorted(created.keys()), dtype=np.int64)
    save_parts(
        os.path.join(HERE, "itemcf_small.npz"),
        click_user=click_df["user_id"].to_numpy(np.int64),
        click_item=click_df["click_article_id"].to_numpy(np.int64),
        click_ts=click_df["click_timestamp"].to_numpy(np.int64),
        created_ids=cids,
        created_vals=np.array([created[c] for c in cids], dtype=np.float64),
        hot=np.array(hot, dtype=np.int64),
        uit_users=np.array(uu, dtype=np.int64),
        uit_offsets=np.array(uoff, dtype=np.int64),
        uit_items=np.array(uitems, dtype=np.int64),
        uit_ts=np.array(uts, dtype=np.int64),
        sim_rows=np.array(rows_i, dtype=np.int64),
        sim_i=np.array(si, dtype=np.int64),
        sim_j=np.array(sj, dtype=np.int64),
        sim_v=np.array(sv, dtype=np.float64),
        recall_users=np.array(ru, dtype=np.int64),
        recall_offsets=np.array(roff, dtype=np.int64),
        recall_items=np.array(ri, dtype=np.int64),
        recall_scores=np.array(rs, dtype=np.float64),
        topk=np.int64(30),
        sim_item_topk=np.int64(cfg30.itemcf_sim_item_topk),
        emb_i=np.array(ei, dtype=np.int64),
        emb_j=np.array(ej, dtype=np.int64),
        emb_v=np.array(ev, dtype=np.float64),
        emb_recall_offsets=np.array(eroff, dtype=np.int64),
        emb_recall_items=np.array(eri, dtype=np.int64),
        emb_recall_scores=np.array(ers, dtype=np.float64),
    )
    print(f"itemcf_small: {len(si)} sim pairs, {len(users)} users recalled")


# --------------------------------------------------------------------------
# YouTubeDNN (youtubednn_recaller.py:86-535)
# --------------------------------------------------------------------------
def gen_youtubednn(tmp):
    import pandas as pd
    import torch
    from nrk.data import synth
    from src.utils.config import RecallConfig
    from src.recall.youtubednn_recaller import YoutubeDNNRecaller

    log = synth.make_click_log(n_users=1000, n_items=5000, seed=11)
    rng = np.random.default_rng(11)
    perm = rng.permutation(len(log))  # click_df row order != time order
    click_df = pd.DataFrame(
        {
            "user_id": log.user_id[perm] * 5 + 3,
            "click_article_id": log.click_article_id[perm] * 3 + 1,
            "click_timestamp": log.click_timestamp[perm],
        }
    )
    cfg = RecallConfig(
        _project_root=tmp,
        youtubednn_embedding_dim=32,
        youtubednn_hidden_units=[64, 32],
        youtubednn_negsample=2,
    )
    seed_all(23)
    rec = YoutubeDNNRecaller(cfg)
    torch.set_num_threads(8)
    rec.train(click_df, epochs=1, batch_size=256, learning_rate=0.01)
    m = rec.model
    users = sorted(rec.user_rawid_2_index.keys()) + [-1]
    res = rec.batch_recall(users, topk=30)
    ri, rs, roff = [], [], [0]
    for u in users:
        for it, sc in res[u]:
            ri.append(it)
            rs.append(sc)
        roff.append(len(ri))
    n_items_enc = len(rec.item_index_2_rawid)
    save_parts(
        os.path.join(HERE, "youtubednn_small.npz"),
        click_user=click_df["user_id"].to_numpy(np.int64),
        click_item=click_df["click_article_id"].to_numpy(np.int64),
        click_ts=click_df["click_timestamp"].to_numpy(np.int64),
        user_emb=m.user_embedding.weight.detach().numpy(),
        item_emb=m.item_embedding.weight.detach().numpy(),
        w0=m.user_tower[0].weight.detach().numpy(),
        b0=m.user_tower[0].bias.detach().numpy(),
        w1=m.user_tower[3].weight.detach().numpy(),
        b1=m.user_tower[3].bias.detach().numpy(),
        user_embeddings=rec.user_embeddings.astype(np.float32),
        item_embeddings=rec.item_embeddings.astype(np.float32),
        user_index_2_rawid=np.array(
            [rec.user_index_2_rawid[i] for i in range(len(rec.user_index_2_rawid))], np.int64
        ),
        item_index_2_rawid=np.array(
            [rec.item_index_2_rawid[i] for i in range(n_items_enc)], np.int64
        ),
        recall_users=np.array(users, dtype=np.int64),
        recall_offsets=np.array(roff, dtype=np.int64),
        recall_items=np.array(ri, dtype=np.int64),
        recall_scores=np.array(rs, dtype=np.float64),
        topk=np.int64(30),
        seq_max_len=np.int64(cfg.youtubednn_seq_max_len),
    )
    print(f"youtubednn_small: {len(users)} users, {n_items_enc} items")


# --------------------------------------------------------------------------
# Brute-force top-K incl. tie stress, through the real recall() (A4 + A5)
# --------------------------------------------------------------------------
def gen_topk(tmp):
    from src.utils.config import RecallConfig
    from src.recall.youtubednn_recaller import YoutubeDNNRecaller

    rng = np.random.default_rng(5)
    d, n_items, k = 32, 5000, 30

    def unit(x):
        x = x.astype(np.float32)
        n = np.linalg.norm(x, axis=1, keepdims=True)
        n[n == 0] = 1
        return (x / n).astype(np.float32)

    # set A: random unit vectors
    items_a = unit(rng.standard_normal((n_items, d)))
    users_a = unit(rng.standard_normal((512, d)))
    # set B: tie stress -- duplicated rows, quantised vectors, all-zero users
    base = unit(rng.standard_normal((64, d)))
    items_b = base[rng.integers(0, 64, size=n_items)]  # heavy exact duplicates
    q = rng.integers(-1, 2, size=(300, d)).astype(np.float32)
    items_b[:300] = unit(q)  # quantised rows -> many equal scores
    users_b = unit(rng.standard_normal((256, d)))
    users_b[:32] = 0.0  # ReLU'd-to-zero users: every score ties at 0
    users_b[32:96] = unit(rng.integers(-1, 2, size=(64, d)))
    users_b[96:128] = base[rng.integers(0, 64, size=32)]

    out = {}
    for tag, users, items in (("a", users_a, items_a), ("b", users_b, items_b)):
        idx = IndexFlatIP(d)
        idx.add(items)
        D, I = idx.search(users, k + 1)
        rec = YoutubeDNNRecaller(RecallConfig(_project_root=tmp, youtubednn_embedding_dim=d))
        rec.model = object()
        rec.user_embeddings = users
        rec.item_embeddings = items
        rec.faiss_index = idx
        rec.user_rawid_2_index = {1000 + u: u for u in range(len(users))}
        # non-identity row->raw mapping exercises the A3 quirk
        raw = rng.permutation(n_items).astype(np.int64) * 2 + 1
        rec.item_index_2_rawid = {r: int(raw[r]) for r in range(n_items)}
        uu = list(rec.user_rawid_2_index.keys()) + [7]
        res = rec.batch_recall(uu, topk=k)
        ri, rs, roff = [], [], [0]
        for u in uu:
            for it, sc in res[u]:
                ri.append(it)
                rs.append(sc)
            roff.append(len(ri))
        out.update(
            {
                f"{tag}_users": users,
                f"{tag}_items": items,
                f"{tag}_D": D,
                f"{tag}_I": I.astype(np.int64),
                f"{tag}_raw": raw,
                f"{tag}_recall_users": np.array(uu, np.int64),
                f"{tag}_recall_offsets": np.array(roff, np.int64),
                f"{tag}_recall_items": np.array(ri, np.int64),
                f"{tag}_recall_scores": np.array(rs, np.float64),
            }
        )
    # k > ntotal: -1 labels / -FLT_MAX scores
    idx = IndexFlatIP(d)
    idx.add(items_a[:10])
    D, I = idx.search(users_a[:4], 16)
    out["small_D"], out["small_I"] = D, I
    out["k"] = np.int64(k)
    save_parts(os.path.join(HERE, "topk_small.npz"), **out)
    print("topk_small: sets a (random) and b (tie stress)")


# --------------------------------------------------------------------------
# EmbeddingSimilarity (similarity/embedding.py:15-67), the 2nd Faiss site
# --------------------------------------------------------------------------
def gen_embsim(tmp):
    import pandas as pd
    from src.utils.config import RecallConfig
    from src.similarity.embedding import EmbeddingSimilarity

    rng = np.random.default_rng(11)
    n_items, d = 1500, 250  # Tianchi articles_emb is 250-d
    emb = rng.standard_normal((n_items, d)).astype(np.float32)
    emb *= rng.uniform(0.2, 5.0, (n_items, 1)).astype(np.float32)
    # exact duplicates (up to scale): "self" is not always column 0 (lower row wins)
    src = rng.integers(0, n_items, 40)
    emb[n_items - 40:] = emb[src] * np.float32(2.0)
    ids = (rng.permutation(n_items).astype(np.int64) * 3 + 5)
    df = pd.DataFrame(emb, columns=[f"emb_{n}" for n in range(d)])
    df.insert(0, "article_id", ids)
    df.index = rng.permutation(n_items) + 10  # reset_index(drop=True) discards this
    cfg = RecallConfig(_project_root=tmp)
    sim = EmbeddingSimilarity(cfg).calculate(df)
    si, sj, sv = [], [], []
    for i, dd in sim.items():
        for j, v in dd.items():
            si.append(i)
            sj.append(j)
            sv.append(v)
    save_parts(
        os.path.join(HERE, "embsim_small.npz"),
        ids=ids, emb=emb, topk=np.int64(cfg.embedding_topk),
        sim_i=np.array(si, np.int64), sim_j=np.array(sj, np.int64), sim_v=np.array(sv, np.float64),
    )
    print(f"embsim_small: {n_items} items x {d}, {len(si)} entries")


# --------------------------------------------------------------------------
# DIN (DIN.py:29-286, 289-520)
# --------------------------------------------------------------------------
USER_FEATS = ["user_click_count", "user_avg_time_gap", "device_group", "avg_click_time", "avg_word_count"]
ITEM_FEATS = ["category_id", "article_popularity", "created_at_ts", "words_count"]
CTX_FEATS = [
    "score", "sim_1", "time_diff_1", "word_diff_1", "sim_2", "time_diff_2", "word_diff_2",
    "sim_3", "time_diff_3", "word_diff_3", "sim_max", "sim_mean", "sim_min", "sim_std",
    "item_user_sim", "recall_in_user_cat",
]


def gen_din(tmp):
    import torch
    from src.rank.DIN import DINModel

    torch.set_num_threads(8)
    uv = dict(zip(USER_FEATS, [38, 121, 7, 501, 91]))
    iv = dict(zip(ITEM_FEATS, [51, 201, 509, 81]))
    cv = {f: 12 for f in CTX_FEATS}
    seed_all(23)
    model = DINModel(uv, iv, cv, embedding_dim=32, attention_hidden_units=[36],
                     mlp_hidden_units=[200, 80], activation="dice").eval()
    sd = {k: v.detach().numpy() for k, v in model.state_dict().items()}

    cap = {}
    model.mlp.register_forward_hook(lambda m, i, o: cap.__setitem__("logit", o.detach()))
    model.activation_unit.register_forward_hook(lambda m, i, o: cap.__setitem__("att", o.detach()))

    rng = np.random.default_rng(29)
    out = {f"sd::{k}": v for k, v in sd.items()}
    T = 50
    for tag, B in (("b512", 512), ("b4096", 4096), ("b37", 37)):
        user = np.stack([rng.integers(0, uv[f], B) for f in USER_FEATS], 1)
        item = np.stack([rng.integers(0, iv[f], B) for f in ITEM_FEATS], 1)
        ctx = np.stack([rng.integers(0, cv[f], B) for f in CTX_FEATS], 1)
        hl = rng.integers(1, T + 1, B)
        hl[rng.random(B) < 0.2] = 0
        mask = (np.arange(T)[None] < hl[:, None]).astype(np.float32)
        hist = np.stack([rng.integers(0, iv[f], (B, T)) for f in ITEM_FEATS], 2)
        hist = hist * (mask[:, :, None] > 0)
        batch = {
            "user_profile": {f: torch.from_numpy(user[:, n].astype(np.int64)) for n, f in enumerate(USER_FEATS)},
            "recall_item": {f: torch.from_numpy(item[:, n].astype(np.int64)) for n, f in enumerate(ITEM_FEATS)},
            "history_items": {f: torch.from_numpy(hist[:, :, n].astype(np.int64)) for n, f in enumerate(ITEM_FEATS)},
            "context": {f: torch.from_numpy(ctx[:, n].astype(np.int64)) for n, f in enumerate(CTX_FEATS)},
            "history_mask": torch.from_numpy(mask),
        }
        with torch.no_grad():
            probs = model(batch).numpy()
        out.update(
            {
                f"{tag}_user": user.astype(np.int16),
                f"{tag}_item": item.astype(np.int16),
                f"{tag}_ctx": ctx.astype(np.int16),
                f"{tag}_hist": hist.astype(np.int16),
                f"{tag}_mask": mask.astype(np.uint8),
                f"{tag}_probs": probs.astype(np.float32),
                f"{tag}_logits": cap["logit"].squeeze(-1).numpy().astype(np.float32),
                f"{tag}_att": cap["att"].squeeze(-1).numpy().astype(np.float32),
            }
        )
    out["user_feats"] = np.array(USER_FEATS)
    out["item_feats"] = np.array(ITEM_FEATS)
    out["ctx_feats"] = np.array(CTX_FEATS)
    save_parts(os.path.join(HERE, "din_small.npz"), **out)
    print("din_small: B in {512, 4096, 37}, T=50")


def gen_din_encode(tmp):
    """Host encoding A14: DINDataset + collate_fn (DIN.py:289-520)."""
    import pandas as pd
    import torch
    from sklearn.preprocessing import LabelEncoder
    from src.rank.DIN import DINDataset, collate_fn

    rng = np.random.default_rng(31)
    n_users, n_items, n_rows, T = 60, 150, 400, 30
    users = [str(u) for u in range(1000, 1000 + n_users)]
    items = [str(i) for i in range(5000, 5000 + n_items)]
    upd = {
        u: {f: float(np.round(rng.random() * 7, 1)) for f in USER_FEATS}
        for u in users[: n_users - 5]  # 5 users without a profile -> all-zero row
    }
    ifd = {
        it: {f: int(rng.integers(0, 12)) for f in ITEM_FEATS} for it in items[: n_items - 10]
    }
    uhd = {}
    for u in users[5:]:  # 5 users without history
        L = int(rng.integers(0, 45))
        uhd[u] = [items[int(x)] for x in rng.integers(0, n_items, L)]
    main = pd.DataFrame(
        {
            "user_id": [int(users[x]) for x in rng.integers(0, n_users, n_rows)],
            "item_id": [int(items[x]) for x in rng.integers(0, n_items, n_rows)],
            "label": rng.integers(0, 2, n_rows),
        }
    )
    for f in CTX_FEATS:
        main[f] = rng.integers(0, 10, n_rows).astype(float)
        main.loc[rng.random(n_rows) < 0.05, f] = 99.0  # unseen bin -> 0
    enc = {}
    for f in USER_FEATS:
        le = LabelEncoder()
        le.fit(list({p[f] for p in upd.values()}))
        enc[f] = le
    for f in ITEM_FEATS:
        le = LabelEncoder()
        le.fit(list({p[f] for p in ifd.values()}))
        enc[f] = le
    fit_rows = main[main[CTX_FEATS[0]] != 99.0]
    for f in CTX_FEATS:
        le = LabelEncoder()
        le.fit(fit_rows[f].fillna(0).astype(str))
        enc[f] = le
    ds = DINDataset(main, upd, ifd, uhd, USER_FEATS, ITEM_FEATS, CTX_FEATS, "label", enc)
    b = collate_fn([ds[i] for i in range(len(ds))], seq_max_len=T)
    # Second case: context columns held as strings -> main_df.iloc[i] is an
    # object row, user_id/item_id stay ints and str() finds the dict keys.
    # (In the float case above the row is upcast to float64, str(user_id) is
    # "1013.0" and every user/item/history feature encodes to 0.)
    main_obj = main.copy()
    for f in CTX_FEATS:
        main_obj[f] = main_obj[f].astype(str)
    ds2 = DINDataset(main_obj, upd, ifd, uhd, USER_FEATS, ITEM_FEATS, CTX_FEATS, "label", enc)
    b2 = collate_fn([ds2[i] for i in range(len(ds2))], seq_max_len=T)
    out = {
        "main_user": main["user_id"].to_numpy(np.int64),
        "main_item": main["item_id"].to_numpy(np.int64),
        "main_label": main["label"].to_numpy(np.int64),
        "main_ctx": main[CTX_FEATS].to_numpy(np.float64),
        "prof_users": np.array([int(u) for u in upd], np.int64),
        "prof_vals": np.array([[upd[u][f] for f in USER_FEATS] for u in upd], np.float64),
        "ifeat_items": np.array([int(i) for i in ifd], np.int64),
        "ifeat_vals": np.array([[ifd[i][f] for f in ITEM_FEATS] for i in ifd], np.int64),
        "hist_users": np.array([int(u) for u in uhd], np.int64),
        "hist_offsets": np.cumsum([0] + [len(v) for v in uhd.values()]).astype(np.int64),
        "hist_items": np.array([int(i) for v in uhd.values() for i in v], np.int64),
        "T": np.int64(T),
        "out_user": np.stack([b["user_profile"][f].numpy() for f in USER_FEATS], 1),
        "out_item": np.stack([b["recall_item"][f].numpy() for f in ITEM_FEATS], 1),
        "out_hist": np.stack([b["history_items"][f].numpy() for f in ITEM_FEATS], 2),
        "out_ctx": np.stack([b["context"][f].numpy() for f in CTX_FEATS], 1),
        "out_mask": b["history_mask"].numpy(),
        "out_labels": b["labels"].numpy(),
        "obj_user": np.stack([b2["user_profile"][f].numpy() for f in USER_FEATS], 1),
        "obj_item": np.stack([b2["recall_item"][f].numpy() for f in ITEM_FEATS], 1),
        "obj_hist": np.stack([b2["history_items"][f].numpy() for f in ITEM_FEATS], 2),
        "obj_ctx": np.stack([b2["context"][f].numpy() for f in CTX_FEATS], 1),
        "obj_mask": b2["history_mask"].numpy(),
    }
    for f in USER_FEATS + ITEM_FEATS + CTX_FEATS:
        out[f"classes::{f}"] = np.array([str(c) for c in enc[f].classes_])
    save_parts(os.path.join(HERE, "din_encode_small.npz"), **out)
    print("din_encode_small: host encoding fixture")


# --------------------------------------------------------------------------
# Rank pipeline drop-in: DINRanker.load -> load_model(load_dir) -> predict
# (DIN.py:529-558, :1328-1399, :1219-1283) on an artifact directory written
# the way the reference's feature step and save_model lay it out
# (config.py:141-161, DIN.py:1285-1326), then rank_and_recommend
# (rank_pipeline.py:143-191).
# --------------------------------------------------------------------------
RP_USERS, RP_ITEMS, RP_ROWS = 70, 160, 400


def rank_pipeline_data(seed):
    """Feature-step outputs of one synthetic data set (plain Python / pandas
    objects, the shapes FeatureExtractor saves): main_df with int context bins
    (so ``main_df.iloc[i]`` is an int64 row and ``str(user_id)`` hits the
    str-keyed dicts), user profiles (float values), item features (int
    values), histories of str item ids (some unknown, some longer than
    din_seq_max_len)."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    users = [str(u) for u in range(2000, 2000 + RP_USERS)]
    items = [str(i) for i in range(7000, 7000 + RP_ITEMS)]
    upd = {u: {f: float(np.round(rng.random() * 6, 1)) for f in USER_FEATS} for u in users[: RP_USERS - 4]}
    ifd = {it: {f: int(rng.integers(0, 15)) for f in ITEM_FEATS} for it in items[: RP_ITEMS - 8]}
    uhd = {}
    for u in users[3:]:
        L = int(rng.integers(0, 42))
        uhd[u] = [items[int(x)] for x in rng.integers(0, RP_ITEMS, L)]
    main = pd.DataFrame({"user_id": [int(users[x]) for x in rng.integers(0, RP_USERS, RP_ROWS)],
                         "item_id": [int(items[x]) for x in rng.integers(0, RP_ITEMS, RP_ROWS)]})
    for f in CTX_FEATS:
        main[f] = rng.integers(0, 10, RP_ROWS)
    main["label"] = rng.integers(0, 2, RP_ROWS)
    lists = {"user_profile_features": list(USER_FEATS), "item_features": list(ITEM_FEATS),
             "context_features": list(CTX_FEATS)}
    return main, upd, ifd, uhd, lists


def write_rank_artifacts(save_path, main, upd, ifd, uhd, lists):
    import pickle

    os.makedirs(save_path, exist_ok=True)
    main.to_csv(os.path.join(save_path, "main_features.csv"), index=False)
    for name, obj in (("user_profile_dict", upd), ("item_features_dict", ifd), ("user_history_dict", uhd),
                      ("feature_lists", lists)):
        with open(os.path.join(save_path, name + ".pkl"), "wb") as f:
            pickle.dump(obj, f)


def gen_rank_pipeline(tmp):
    import pickle

    import pandas as pd
    import torch
    from src.rank.DIN import DINModel, DINRanker
    from src.utils.config import RankConfig

    torch.set_num_threads(8)
    out = {}
    for dim in (32, 16, 64):
        root = os.path.join(tmp, f"rank_{dim}")
        main, upd, ifd, uhd, lists = rank_pipeline_data(41 + dim)
        cfg = RankConfig(_project_root=root, din_embedding_dim=dim, batch_size=128, num_workers=0,
                         pin_memory=False)
        write_rank_artifacts(cfg.save_path, main, upd, ifd, uhd, lists)
        # the trained model: reference vocabularies, reference init (seeded),
        # saved with the reference's own save_model + the encoders train() pickles
        r0 = DINRanker(cfg)
        r0.load()
        uv, iv, cv = r0._prepare_vocab_dicts()
        seed_all(23 + dim)
        r0.model = DINModel(uv, iv, cv, embedding_dim=dim, attention_hidden_units=[36],
                            mlp_hidden_units=[200, 80], activation="dice")
        with torch.no_grad():  # spread the attention weights so the history matters
            r0.model.activation_unit.mlp[0].weight.mul_(4.0)
        r0.save_model(cfg.save_path)
        with open(os.path.join(cfg.save_path, "label_encoders.pkl"), "wb") as f:
            pickle.dump(r0.label_encoders, f)
        sd = torch.load(os.path.join(cfg.save_path, "din_model.pth"), weights_only=True)
        # the reference's serving path, executed: RankPipeline.load_model
        # (rank_pipeline.py:96-103) then predict() at two batch sizes
        probs = {}
        for bs in (128, 100):
            r = DINRanker(RankConfig(_project_root=root, din_embedding_dim=dim, batch_size=bs, num_workers=0,
                                     pin_memory=False))
            r.load()
            r.load_model(load_dir=cfg.save_path)
            probs[bs] = r.predict().astype(np.float32)
        # rank_and_recommend (rank_pipeline.py:162-174), top_k = 5 on the bs-128 scores
        df = pd.read_csv(cfg.main_features_path)
        df["rank_score"] = probs[128]
        rec_u, rec_i, rec_s = [], [], []
        for user_id, group in df.groupby("user_id"):
            top = group.nlargest(5, "rank_score")[["item_id", "rank_score"]]
            for _, row in top.iterrows():
                rec_u.append(str(user_id))
                rec_i.append(str(row["item_id"]))
                rec_s.append(float(row["rank_score"]))
        p = f"d{dim}_"
        out.update({p + k: v for k, v in (
            ("main", main[["user_id", "item_id"] + CTX_FEATS + ["label"]].to_numpy(np.int64)),
            ("prof_users", np.array(list(upd), dtype=str)),
            ("prof_vals", np.array([[upd[u][f] for f in USER_FEATS] for u in upd], np.float64)),
            ("ifeat_items", np.array(list(ifd), dtype=str)),
            ("ifeat_vals", np.array([[ifd[i][f] for f in ITEM_FEATS] for i in ifd], np.int64)),
            ("hist_users", np.array(list(uhd), dtype=str)),
            ("hist_offsets", np.cumsum([0] + [len(v) for v in uhd.values()]).astype(np.int64)),
            ("hist_items", np.array([i for v in uhd.values() for i in v], dtype=str)),
            ("probs_bs128", probs[128]), ("probs_bs100", probs[100]),
            ("rec_user", np.array(rec_u, dtype=str)), ("rec_item", np.array(rec_i, dtype=str)),
            ("rec_score", np.array(rec_s, np.float64)))})
        out.update({f"{p}sd::{k}": v.numpy() for k, v in sd.items()})
        for f, le in r0.label_encoders.items():  # object (str) classes stored as a unicode array
            c = np.asarray(le.classes_)
            out[f"{p}classes::{f}"] = c.astype(str) if c.dtype == object else c
    out["user_feats"], out["item_feats"], out["ctx_feats"] = (np.array(USER_FEATS), np.array(ITEM_FEATS),
                                                               np.array(CTX_FEATS))
    save_parts(os.path.join(HERE, "rank_pipeline_small.npz"), **out)
    print("rank_pipeline_small: DINRanker.load/load_model/predict at D in {32, 16, 64}, bs 128 / 100")


# --------------------------------------------------------------------------
# RecallFusion.fuse (fusion.py:67-342), every strategy x normalisation
# --------------------------------------------------------------------------
def fusion_inputs():
    """Synthetic recall dicts shaped like RecallPipeline's (itemcf with its
    negative hot-fill scores, youtubednn, a third method), with overlaps,
    repeated items inside a list, empty and one-entry lists, equal scores
    (ties) and users present in only some methods."""
    rng = np.random.default_rng(13)
    users = (rng.permutation(400) * 5 + 1000).tolist()
    pool = rng.permutation(3000) * 3 + 7
    methods = {}
    for name, n_u, scale in (("itemcf", 320, 3.0), ("youtubednn", 300, 1.0), ("usercf", 150, 0.5)):
        res = {}
        for u in rng.choice(users, n_u, replace=False).tolist():
            L = int(rng.choice([0, 1, 2, 5, 20, 30, 30, 30]))
            its = pool[rng.integers(0, 120, L)].tolist()  # small pool per user: overlaps and repeats
            sc = np.round(rng.standard_normal(L) * scale, 2)  # rounding makes ties
            if name == "itemcf" and L > 3:
                sc[-2:] = [-(its[-2] % 50) - 100.0, -(its[-1] % 50) - 100.0]  # hot fill (:116-122)
            if name == "youtubednn":
                sc = sc.astype(np.float32).astype(np.float64)
            res[u] = [(int(i), float(s)) for i, s in zip(its, sc)]
        methods[name] = res
    weights = {"itemcf": 1.0, "youtubednn": 0.8, "usercf": 0.5}
    history = {u: set(pool[rng.integers(0, 120, 8)].tolist()) for u in users[:200]}
    return methods, weights, history


def _flat_dict(d):
    keys = list(d.keys())
    lens = [len(d[k]) for k in keys]
    items = [t[0] for k in keys for t in d[k]]
    scores = [t[1] for k in keys for t in d[k]]
    return (np.array(keys, np.int64), np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
            np.array(items, np.int64), np.array(scores, np.float64))


def gen_fusion(tmp):
    from src.utils.config import RecallConfig
    from src.recall.fusion import RecallFusion

    methods, weights, history = fusion_inputs()
    out = {"methods": np.array(list(methods)), "weights": np.array([weights[m] for m in methods])}
    for m, d in methods.items():
        out[f"in::{m}::users"], out[f"in::{m}::offsets"], out[f"in::{m}::items"], out[f"in::{m}::scores"] = \
            _flat_dict(d)
    hu = list(history)
    out["hist_users"] = np.array(hu, np.int64)
    out["hist_offsets"] = np.concatenate([[0], np.cumsum([len(history[u]) for u in hu])]).astype(np.int64)
    out["hist_items"] = np.array([i for u in hu for i in sorted(history[u])], np.int64)
    cases = [(s, n, False) for s in ("weighted_sum", "weighted_avg", "max_score", "harmonic_mean",
                                     "diversity_weighted", "rrf") for n in ("local", "global", "z-score")]
    cases.append(("weighted_avg", "global", True))
    for strat, norm, seen in cases:
        f = RecallFusion(RecallConfig(_project_root=tmp), fusion_strategy=strat, normalize_method=norm)
        for m, d in methods.items():
            f.add_recall_result(m, d, weight=weights[m])
        res = f.fuse(topk=30, user_history=history if seen else None, remove_seen=seen)
        tag = f"out::{strat}::{norm}::{int(seen)}"
        out[tag + "::users"], out[tag + "::offsets"], out[tag + "::items"], out[tag + "::scores"] = \
            _flat_dict(res)
    save_parts(os.path.join(HERE, "fusion_small.npz"), **out)


# --------------------------------------------------------------------------
# Context features (feature_extractor.py:440-723), binning (:838-898),
# context label encoders (DIN.py:560-617) and the dataset's codes (:330-353)
# --------------------------------------------------------------------------
CTX_FEATS = ["score", "sim_1", "time_diff_1", "word_diff_1", "sim_2", "time_diff_2", "word_diff_2",
             "sim_3", "time_diff_3", "word_diff_3", "sim_max", "sim_mean", "sim_min", "sim_std",
             "item_user_sim", "recall_in_user_cat"]


def ctxfeat_inputs():
    """Synthetic inputs of FeatureExtractor._extract_context_features: the
    dicts load_data builds (str item ids), a train click log, and a recall
    main_df.  Gaps on purpose: items missing from each dict, all-zero content
    rows, users without history / without a YouTubeDNN vector, users with
    fewer than last_N history items."""
    import pandas as pd

    rng = np.random.default_rng(31)
    n_items, n_users, dw, dy = 600, 260, 64, 64  # dy = embedding_dim: the zero default (:523) is that wide
    ids = [str(i * 7 + 3) for i in range(n_items)]
    keep = lambda frac: [i for i in ids if rng.random() < frac]  # noqa: E731
    w2v = {i: rng.standard_normal(dw).astype(np.float32) * 0.3 for i in keep(0.92)}
    content = {i: rng.standard_normal(250).astype(np.float64) for i in keep(0.9)}
    for i in list(content)[:12]:
        content[i] = np.zeros(250)  # an all-zero content row (word_diff -> 0)
    created = {i: np.float64(rng.random()) for i in keep(0.9)}
    ctype = {i: int(rng.integers(0, 8)) for i in keep(0.95)}
    art_yt = {i: rng.standard_normal(dy).astype(np.float32) for i in keep(0.9)}
    users = [int(u) for u in rng.permutation(5000)[:n_users] + 10]
    rows = []
    for u in users[:220]:  # the last 40 users have no clicks (no history)
        L = int(rng.integers(1, 9))
        its = rng.integers(0, n_items, L)
        ts = 1_507_000_000_000 + np.cumsum(rng.integers(1, 10_000, L))
        rows += [(u, int(ids[i]), int(t)) for i, t in zip(its, ts)]
    click = pd.DataFrame(rows, columns=["user_id", "click_article_id", "click_timestamp"])
    user_yt = {str(u): rng.standard_normal(dy).astype(np.float32) for u in users if rng.random() < 0.85}
    mrows = []
    for u in users:
        for i in rng.integers(0, n_items + 40, int(rng.integers(5, 31))):  # ids >= n_items: unknown items
            iid = ids[i] if i < n_items else str(100_000 + int(i))
            mrows.append((str(u), iid, float(np.round(rng.random(), 3))))
    main_df = pd.DataFrame(mrows, columns=["user_id", "item_id", "score"])
    return dict(w2v=w2v, content=content, created=created, ctype=ctype, art_yt=art_yt, user_yt=user_yt,
                click=click, main_df=main_df)


def gen_ctxfeat(tmp):
    import types as _types

    import pandas as pd

    # gensim (Word2Vec) is not installed: a stand-in module satisfies the
    # import; Word2Vec itself is never called -- the article-id vectors are
    # an input here (_get_article_id_embeddings is replaced by the dict).
    gm = _types.ModuleType("gensim")
    gmm = _types.ModuleType("gensim.models")
    gmm.Word2Vec = None
    gm.models = gmm
    sys.modules.setdefault("gensim", gm)
    sys.modules.setdefault("gensim.models", gmm)
    from src.utils.config import RecallConfig, RankConfig
    from src.features.feature_extractor import FeatureExtractor
    from src.rank.DIN import DINRanker, DINDataset

    inp = ctxfeat_inputs()
    fe = FeatureExtractor(RecallConfig(_project_root=tmp))
    fe.train_click_df = inp["click"]
    fe.main_df = inp["main_df"].copy()
    fe.article_type_dict = inp["ctype"]
    fe.article_content_emb_dict = inp["content"]
    fe.article_created_time_dict = inp["created"]
    fe.user_youtubednn_emb_dict = inp["user_yt"]
    fe.article_youtubednn_emb_dict = inp["art_yt"]
    fe._get_article_id_embeddings = lambda: inp["w2v"]
    fe._extract_context_features()
    assert fe.context_features == CTX_FEATS
    raw = fe.main_df[CTX_FEATS].copy()
    fe._apply_binning()
    binned = fe.main_df[CTX_FEATS].copy()
    ns = _types.SimpleNamespace(user_profile_dict={}, item_features_dict={}, main_df=fe.main_df,
                                context_features=CTX_FEATS, user_profile_features=[], item_features=[],
                                label_encoders={})
    DINRanker._prepare_vocab_dicts(ns)
    ds = DINDataset(fe.main_df, {}, {}, fe.user_history_dict, [], [], CTX_FEATS, label_col="score",
                    label_encoders=ns.label_encoders)
    codes = np.array([[ds[i]["context"][f] for f in CTX_FEATS] for i in range(len(fe.main_df))], np.int64)
    out = {"ctx_feats": np.array(CTX_FEATS)}
    for k in ("w2v", "content", "created", "ctype", "art_yt", "user_yt"):
        d = inp[k]
        out[f"in::{k}::keys"] = np.array(list(d.keys()))
        out[f"in::{k}::vals"] = np.array(list(d.values()))
    for c in ("user_id", "click_article_id", "click_timestamp"):
        out[f"in::click::{c}"] = inp["click"][c].to_numpy(np.int64)
    out["in::main::user_id"] = inp["main_df"]["user_id"].to_numpy().astype(str)
    out["in::main::item_id"] = inp["main_df"]["item_id"].to_numpy().astype(str)
    out["in::main::score"] = inp["main_df"]["score"].to_numpy(np.float64)
    hu = list(fe.user_history_dict)
    out["hist_users"] = np.array(hu)
    out["hist_offsets"] = np.concatenate([[0], np.cumsum([len(fe.user_history_dict[u]) for u in hu])])
    out["hist_items"] = np.array([i for u in hu for i in fe.user_history_dict[u]])
    for f in CTX_FEATS:
        out[f"raw::{f}"] = raw[f].to_numpy()
        out[f"binned::{f}"] = binned[f].to_numpy()
        if f in fe.discretizers:
            out[f"edges::{f}"] = np.asarray(fe.discretizers[f].bin_edges_[0], np.float64)
        out[f"classes::{f}"] = np.asarray(ns.label_encoders[f].classes_).astype(str)
    out["codes"] = codes
    save_parts(os.path.join(HERE, "ctxfeat_small.npz"), **out)


def main():
    import_reference()
    tmp = tempfile.mkdtemp(prefix="nrk_golden_")
    gen_topk(tmp)
    gen_itemcf(tmp)
    gen_youtubednn(tmp)
    gen_din(tmp)
    gen_din_encode(tmp)
    gen_embsim(tmp)
    gen_fusion(tmp)
    gen_ctxfeat(tmp)
    gen_rank_pipeline(tmp)


if __name__ == "__main__":
    if len(sys.argv) > 1:  # regenerate selected fixtures: make_golden.py fusion embsim ...
        import_reference()
        tmp = tempfile.mkdtemp(prefix="nrk_golden_")
        for name in sys.argv[1:]:
            globals()["gen_" + name](tmp)
    else:
        main()

"""Time UserCF on a synthetic log (informational; bench.py has no UserCF leg).

usage: python tools/usercf_time.py --users N [--items 364047] [--topk 10]

Runs UserCFSimilarity.compute() (the direct top-n, nrk_usercf_topn) and
UserCFRecaller.batch_recall of every user on synth.make_click_log(N, items,
seed=23), and prints sum n_i^2 (the pair terms the reference's loop would
add), the device time of each and the adds per second.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "news-recommendation-tc_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, required=True)
    ap.add_argument("--items", type=int, default=364047)
    ap.add_argument("--topk", type=int, default=10)
    a = ap.parse_args()
    import pandas as pd
    import torch

    from nrk import ops
    from nrk.config import RecallConfig
    from nrk.data import extractors, synth
    from nrk.recall.usercf_recaller import UserCFRecaller
    from nrk.similarity.user_cf import UserCFSimilarity

    log = synth.make_click_log(a.users, a.items, seed=23)
    art = synth.make_articles(a.items, seed=23)
    df = pd.DataFrame({"user_id": log.user_id, "click_article_id": log.click_article_id,
                       "click_timestamp": log.click_timestamp})
    n_i = np.bincount(log.click_article_id)
    terms = int((n_i.astype(np.int64) ** 2).sum())
    print(f"users {a.users}  clicks {len(df)}  hottest item {int(n_i.max())} clickers  sum n_i^2 {terms:.4g}",
          flush=True)
    cfg = RecallConfig()
    act = extractors.user_activate_degree(df)
    calc = UserCFSimilarity(cfg)
    t0 = time.perf_counter()
    res = calc.compute(df, act)
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    # the kernels alone, on the inputs compute() laid out
    ws = torch.empty(ops._lib.lib().nrk_usercf_workspace_bytes(len(res.user_ids), len(df), cfg.usercf_sim_user_topk),
                     dtype=torch.uint8, device="cuda")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    ops.usercf_topn(*res._inputs, topn=cfg.usercf_sim_user_topk, workspace=ws)
    ev1.record()
    torch.cuda.synchronize()
    t_k = ev0.elapsed_time(ev1) / 1e3
    nnz = res.nnz.to(torch.int64)
    print(f"compute(): {t_all:.3f} s with the host layout; nrk_usercf_topn {t_k:.4f} s = {terms / t_k:.4g} adds/s; "
          f"workspace {ws.numel() / 2**30:.2f} GiB; u2u entries (never stored) {int(nnz.sum())}, "
          f"max row {int(nnz.max())}", flush=True)
    del ws
    users, off, items, ts = extractors.user_item_time_csr(df)
    uit = extractors.csr_to_dict(users, off, items, ts)
    created = dict(zip(art.article_id.tolist(), synth.minmax_created(art).tolist()))
    hot = extractors.item_topk_click(df, k=50)
    t0 = time.perf_counter()
    rec = UserCFRecaller.from_result(cfg, res, uit, created, hot)
    t_build = time.perf_counter() - t0
    q = list(uit)
    t0 = time.perf_counter()
    out = rec.batch_recall(q, topk=a.topk)
    t_rec = time.perf_counter() - t0
    print(f"UserCFRecaller: build {t_build:.3f} s (host), batch_recall of {len(q)} users top-{a.topk} "
          f"{t_rec:.3f} s with the host lists ({len(q) / t_rec:.4g} users/s); first list {out[q[0]][:3]}",
          flush=True)


if __name__ == "__main__":
    main()

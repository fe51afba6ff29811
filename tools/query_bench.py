"""ops.ip_query against ops.ip_topk for small user batches, same process, same card.

usage: python tools/query_bench.py [--out FILE] [--skip-large]

Points: n_users in {1, 8, 64, 512, 2048, 4096} on a config-2-shaped catalog
(364,047 x 32 unit rows, k = 31) and n_users in {1, 64} at 5M x 128.  Per point
and path: device events around every launch, 5 warm-up + 20 timed launches,
the two paths interleaved over three rounds (60 timed launches each); median
and range in microseconds.  Both paths run with a preallocated workspace and
without the finite check (no host sync inside the timed span), and their
outputs are compared once per point.

The last column says whether EVERY ip_query launch was faster than EVERY
ip_topk launch: YoutubeDNNRecaller.query_max_users is half the largest
config-2 n_users with a yes.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "news-recommendation-tc_amd"))

WARMUP, TIMED, ROUNDS = 5, 20, 3


def timed(fn):
    import torch

    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(TIMED):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def point(ops, cat, n_users, k, emit):
    import torch

    g = torch.Generator(device="cuda").manual_seed(n_users)
    users = torch.nn.functional.normalize(torch.randn((n_users, cat.d), device="cuda", generator=g), dim=1).contiguous()
    ws_q = ops.ip_query_workspace(n_users, cat, k, "cuda")
    ws_t = ops.ip_topk_workspace(n_users, cat, k, "cuda")
    run_q = lambda: ops.ip_query(users, cat, k, exact=True, workspace=ws_q, check_finite=False)  # noqa: E731
    run_t = lambda: ops.ip_topk(users, cat, k, exact=True, workspace=ws_t, check_finite=False)  # noqa: E731
    same = all(torch.equal(a, b) for a, b in zip(run_q(), run_t()))
    tq, tt = [], []
    for _ in range(ROUNDS):
        tq += timed(run_q)
        tt += timed(run_t)
    plan = ops.ip_query_plan(n_users, cat.n, cat.d, k)
    below = max(tq) < min(tt)
    emit(f"{cat.n:>9} x {cat.d:<3} k={k} users={n_users:<5} G={plan[2]:<4} "
         f"ip_query {statistics.median(tq):10.1f} us [{min(tq):.1f} .. {max(tq):.1f}]   "
         f"ip_topk {statistics.median(tt):10.1f} us [{min(tt):.1f} .. {max(tt):.1f}]   "
         f"x{statistics.median(tt) / statistics.median(tq):.1f}  outputs {'equal' if same else 'DIFFER'}  "
         f"every query run below every topk run: {'yes' if below else 'no'}")
    return below


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 5M x 128 catalog")
    a = ap.parse_args()
    import torch

    from nrk import ops

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    emit(f"# tools/query_bench.py: {torch.cuda.get_device_name(0)}; device events, {WARMUP} warm-up + {TIMED} timed "
         f"launches per path, interleaved over {ROUNDS} rounds; us per launch: median [min .. max]")

    def catalog(n, d):
        g = torch.Generator(device="cuda").manual_seed(n + d)
        return ops.Catalog(torch.nn.functional.normalize(torch.randn((n, d), device="cuda", generator=g),
                                                         dim=1).contiguous())

    cat = catalog(364047, 32)
    best = 0
    for n in (1, 8, 64, 512, 2048, 4096):
        if point(ops, cat, n, 31, emit):
            best = n
    emit(f"# config-2 catalog: largest n_users with every ip_query run below every ip_topk run = {best}; "
         f"query_max_users = {best // 2}")
    del cat
    if not a.skip_large:
        cat = catalog(5_000_000, 128)
        for n in (1, 64):
            point(ops, cat, n, 31, emit)


if __name__ == "__main__":
    main()

"""GPU parity of ops.ip_query, the catalog-split top-k for small user batches.

Checker = the CPU oracle (oracle.ip_topk, exact=True), the golden fixtures and
ops.ip_topk itself.  Every comparison is exact equality: rows, fp32 scores and
fp64 scores.  The boundary shapes come from ops.ip_query_plan (users per tile,
items per round, workgroups along the catalog), not from constants copied here.
"""
import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu

D, K = 32, 31
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def _unit(x):
    n = np.linalg.norm(x, axis=1, keepdims=True)
    n[n == 0] = 1
    return (x / n).astype(np.float32)


def _host(s, r, e):
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy().astype(np.int64), e.cpu().numpy()


def _run_query(ops, users, items, k, row_offset=0, workspace=None):
    cat = ops.Catalog(_dev(items, torch.float32))
    return _host(*ops.ip_query(_dev(users, torch.float32), cat, k, row_offset=row_offset, exact=True,
                               workspace=workspace))


def _check_vs_oracle(got, users, items, k, row_offset=0):
    s, r, e = got
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    real = ro >= 0
    assert np.array_equal(r, np.where(real, ro + row_offset, -1))
    assert np.array_equal(s, so)
    assert np.array_equal(e[real], eo[real])
    # past min(k, n_items): the exact path's padding
    assert np.all(s[~real] == -FLT_MAX) and np.all(np.isneginf(e[~real]))


def _plan(ops, n_users, d=D, k=K):
    """(UQ, items per round, G at a catalog long enough for the full grid)."""
    uq, rnd, g, _ = ops.ip_query_plan(n_users, 2 ** 29, d, k)
    return uq, rnd, g


def _data(n_users, n_items, d, seed):
    rng = np.random.default_rng(seed)
    return _unit(rng.standard_normal((n_users, d))), _unit(rng.standard_normal((n_items, d)))


# ------------------------------------------------------- boundary shapes --
@pytest.mark.parametrize("which", ["1", "UQ-1", "UQ", "UQ+1", "3UQ+1"])
def test_user_tile_boundaries(ops, which):
    uq = _plan(ops, 1)[0]
    n_users = {"1": 1, "UQ-1": uq - 1, "UQ": uq, "UQ+1": uq + 1, "3UQ+1": 3 * uq + 1}[which]
    assert n_users >= 1
    users, items = _data(n_users, 3001, D, 100 + n_users)
    _check_vs_oracle(_run_query(ops, users, items, K), users, items, K)


@pytest.mark.parametrize("which", ["1", "30", "R-1", "R", "R+1", "G*R", "G*R+1"])
@pytest.mark.parametrize("n_users", [1, 9])
def test_item_round_boundaries(ops, which, n_users):
    """One item; fewer items than k (padding); around one round; and G rounds
    exactly / plus the first item of workgroup 0's second round."""
    _, rnd, g = _plan(ops, n_users)
    n_items = {"1": 1, "30": 30, "R-1": rnd - 1, "R": rnd, "R+1": rnd + 1, "G*R": g * rnd, "G*R+1": g * rnd + 1}[which]
    assert ops.ip_query_plan(n_users, n_items, D, K)[2] == min(g, -(-n_items // rnd))
    users, items = _data(n_users, n_items, D, 200 + len(which) + n_users)
    got = _run_query(ops, users, items, K)
    _check_vs_oracle(got, users, items, K)
    if which == "30":
        assert np.all(got[1][:, 30:] == -1) and np.all(got[1][:, :30] >= 0)


@pytest.mark.parametrize("d", [16, 32, 50, 64, 100, 128, 250, 256, 1, 3, 36])
def test_dims(ops, d):
    """Whole 32-wide steps (32, 64, 128, 256), float4 tails after them or
    alone (16, 100, 36), scalar rows (50, 250, 1, 3)."""
    users, items = _data(11, 3000, d, 300 + d)
    _check_vs_oracle(_run_query(ops, users, items, 21), users, items, 21)


@pytest.mark.parametrize("k", [1, 2, 64, 128])
def test_k_range(ops, k):
    users, items = _data(10, 3000, D, 400 + k)
    users[0] = 0.0  # an all-tie row
    _check_vs_oracle(_run_query(ops, users, items, k), users, items, k)


def test_k_128_many_rounds(ops):
    """k = 128 with workgroups that run many rounds: the list is cut to 128
    again and again, with only one round of spare capacity."""
    n_users = 40  # 5 tiles: a shorter catalog axis, more rounds per workgroup
    _, rnd, g = _plan(ops, n_users)
    users, items = _data(n_users, 7 * g * rnd + 77, D, 77)
    _check_vs_oracle(_run_query(ops, users, items, 128), users, items, 128)


def test_larger_catalog(ops):
    users, items = _data(9, 600_011, D, 5)
    _check_vs_oracle(_run_query(ops, users, items, K), users, items, K)


# ------------------------------------------------------------------ ties --
@pytest.mark.parametrize("tag", ["a", "b"])
def test_golden_ties(ops, golden, tag):
    """Duplicated rows, quantised vectors and all-zero users (the reference's
    own search results)."""
    g = golden("topk_small")
    k = int(g["k"]) + 1
    s, r, _ = _run_query(ops, g[f"{tag}_users"], g[f"{tag}_items"], k)
    assert np.array_equal(r, g[f"{tag}_I"])
    assert np.array_equal(s, g[f"{tag}_D"])


def test_golden_padding(ops, golden):
    g = golden("topk_small")
    k = g["small_I"].shape[1]
    s, r, e = _run_query(ops, g["a_users"][:4], g["a_items"][:10], k)
    assert np.array_equal(r, g["small_I"])
    assert np.array_equal(s, g["small_D"])
    assert np.all(np.isneginf(e[:, 10:])) and np.all(np.isfinite(e[:, :10]))


def test_all_zero_user_keeps_the_first_rows(ops):
    _, rnd, g = _plan(ops, 1)
    items = _data(1, 4 * g * rnd, D, 6)[1]
    s, r, e = _run_query(ops, np.zeros((1, D), np.float32), items, K)
    assert np.array_equal(r, np.arange(K)[None])
    assert np.all(s == 0) and np.all(e == 0) and not np.signbit(e).any()


def test_duplicate_rows_across_workgroups(ops):
    """Every score exists in every catalog workgroup's slice: the merge's
    order decides, lower rows first."""
    _, rnd, g = _plan(ops, 3)
    base = _data(1, 50, D, 7)[1]
    rng = np.random.default_rng(8)
    items = base[rng.integers(0, 50, size=3 * g * rnd + 5)]
    users = np.concatenate([base[:2], np.zeros((1, D), np.float32)])
    _check_vs_oracle(_run_query(ops, users, items, K), users, items, K)


# ------------------------------------------- equality with the scan path --
@pytest.fixture(scope="module")
def same_inputs(ops):
    users, items = _data(200, 20_000, D, 9)
    users[3] = 0.0
    items[100:110] = items[5]
    return _dev(users), ops.Catalog(_dev(items))


@pytest.mark.parametrize("row_offset", [0, 12345])
def test_equals_ip_topk(ops, same_inputs, row_offset):
    users, cat = same_inputs
    q = _host(*ops.ip_query(users, cat, K, row_offset=row_offset, exact=True))
    t = _host(*ops.ip_topk(users, cat, K, row_offset=row_offset, exact=True))
    for a, b in zip(q, t):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    assert q[1].min() >= row_offset
    s2, r2 = ops.ip_query(users, cat, K, row_offset=row_offset)  # without the fp64 output
    assert np.array_equal(s2.cpu().numpy(), q[0]) and np.array_equal(r2.cpu().numpy(), q[1])


# ------------------------------------------------------- workspace reuse --
def test_workspace_reuse_and_stale_contents(ops):
    users, items = _data(19, 5000, D, 10)
    cat = ops.Catalog(_dev(items))
    ws = ops.ip_query_workspace(19, cat, K, "cuda")
    assert ws.numel() >= ops.ip_query_workspace(5, cat, K, "cuda").numel()
    ws.fill_(0xFF)
    before = ws.data_ptr()
    for n in (19, 5, 19):
        got = _host(*ops.ip_query(_dev(users[:n]), cat, K, exact=True, workspace=ws))
        fresh = _host(*ops.ip_query(_dev(users[:n]), cat, K, exact=True))
        for a, b in zip(got, fresh):
            assert np.array_equal(a, b)
        _check_vs_oracle(got, users[:n], items, K)
    assert ws.data_ptr() == before


def test_no_users_and_no_items(ops):
    cat = ops.Catalog(_dev(_data(1, 100, D, 11)[1]))
    s, r, e = ops.ip_query(torch.empty((0, D), device="cuda"), cat, K, exact=True)
    assert s.shape == (0, K) and r.shape == (0, K) and e.shape == (0, K)
    empty = ops.Catalog(torch.empty((0, D), device="cuda"))
    s, r, e = _host(*ops.ip_query(_dev(_data(3, 1, D, 12)[0]), empty, K, exact=True))
    assert np.all(s == -FLT_MAX) and np.all(r == -1) and np.all(np.isneginf(e))


def test_nonfinite_users_rejected_on_device(ops):
    cat = ops.Catalog(_dev(_data(1, 100, D, 13)[1]))
    u = torch.zeros((2, D), device="cuda")
    u[1, 3] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        ops.ip_query(u, cat, K)


# ---------------------------------------------------------------- plugin --
@pytest.fixture(scope="module")
def recaller(golden):
    from nrk.recall.youtubednn_recaller import YoutubeDNNRecaller

    g = golden("youtubednn_small")
    return YoutubeDNNRecaller.from_embeddings(g["user_embeddings"], g["item_embeddings"],
                                              user_index_2_rawid=g["user_index_2_rawid"],
                                              item_index_2_rawid=g["item_index_2_rawid"])


@pytest.fixture
def spy(ops, monkeypatch):
    calls = []
    real = ops.ip_query

    def wrapped(users, *a, **kw):
        calls.append(int(users.shape[0]))
        return real(users, *a, **kw)

    monkeypatch.setattr(ops, "ip_query", wrapped)
    return calls


def test_recaller_takes_the_query_path_for_small_batches(recaller, spy, golden):
    from nrk.recall.youtubednn_recaller import YoutubeDNNRecaller

    g = golden("youtubednn_small")
    k = int(g["topk"])
    uids = [int(u) for u in g["recall_users"][:5]]
    assert "query_max_users" not in vars(recaller) and YoutubeDNNRecaller.query_max_users >= 5
    one_q, five_q = recaller.recall(uids[0], topk=k), recaller.batch_recall(uids, topk=k)
    assert spy == [1, 5]
    try:
        recaller.query_max_users = 0  # today's path exactly
        one_t, five_t = recaller.recall(uids[0], topk=k), recaller.batch_recall(uids, topk=k)
        assert spy == [1, 5]
    finally:
        del recaller.query_max_users
    assert one_q == one_t and five_q == five_t and list(five_q) == uids
    ro = g["recall_offsets"]
    for n, u in enumerate(uids):
        assert [a for a, _ in five_q[u]] == g["recall_items"][ro[n]:ro[n + 1]].tolist()
        assert [b for _, b in five_q[u]] == g["recall_scores"][ro[n]:ro[n + 1]].tolist()
    assert one_q == five_q[uids[0]]
    assert recaller.recall(10 ** 9, topk=5) == [] and spy == [1, 5]  # unknown user: no search at all


def test_recaller_keeps_ip_topk_beyond_k_128_and_above_the_limit(recaller, spy, golden):
    g = golden("youtubednn_small")
    uids = [int(u) for u in g["recall_users"][:5]]
    wide = recaller.batch_recall(uids, topk=128)  # a 129-deep search
    assert spy == [] and all(len(v) == 128 for v in wide.values())
    recaller.batch_recall(uids, topk=127)
    assert spy == [5]
    try:
        recaller.query_max_users = 4
        recaller.batch_recall(uids, topk=30)
        assert spy == [5]
        recaller.batch_recall(uids[:4], topk=30)
        assert spy == [5, 4]
    finally:
        del recaller.query_max_users

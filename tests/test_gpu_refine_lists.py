"""GPU parity of the refine's list mode: after a plain screen the finish
compacts the scan's two append lists itself (cut = the scan's list bound
- 2 eps); after nrk_ip_topk_bound it reads the select's band.  Every case
compares rows, fp32 scores and fp64 scores with oracle.ip_topk bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nrk import ops as _ops

    return _ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _unit(x):
    n = np.linalg.norm(x, axis=1, keepdims=True)
    n[n == 0] = 1
    return (x / n).astype(np.float32)


def _check(ops, users, items, k):
    cat = ops.Catalog(_dev(items))
    s, r, e = ops.ip_topk(_dev(users), cat, k, exact=True)
    s2, r2 = ops.ip_topk(_dev(users), cat, k)  # the fp32-key sort of k <= 64
    torch.cuda.synchronize()
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy(), eo)
    assert np.array_equal(r2.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s2.cpu().numpy(), so)


@pytest.fixture(scope="module")
def random_case():
    """301 users (the last workgroup holds one) x 20,000 items per dim, and
    the oracle's result per (dim, k), computed once."""
    data, ref = {}, {}

    def get(d, k):
        if d not in data:
            rng = np.random.default_rng(1000 + d)
            data[d] = (_unit(rng.standard_normal((301, d))), _unit(rng.standard_normal((20_000, d))))
        if (d, k) not in ref:
            ref[d, k] = oracle.ip_topk(*data[d], k, exact=True)
        return data[d], ref[d, k]

    return get


@pytest.mark.parametrize("k", [1, 10, 31, 64, 100])
@pytest.mark.parametrize("d", [16, 32, 64, 128, 250])
def test_list_mode_random_vs_oracle(ops, random_case, d, k):
    (users, items), (so, ro, eo) = random_case(d, k)
    cat = ops.Catalog(_dev(items))
    s, r, e = ops.ip_topk(_dev(users), cat, k, exact=True)
    s2, r2 = ops.ip_topk(_dev(users), cat, k)
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy(), eo)
    assert np.array_equal(r2.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s2.cpu().numpy(), so)


def _rising(n_items, n_users, seed):
    """Users close to one direction, item scores rising with the row: every
    half-block is a new record for every user, so each lane's append list
    grows to about the block count."""
    rng = np.random.default_rng(seed)
    d = 32
    axis = _unit(rng.standard_normal((1, d)))[0]
    users = _unit(axis[None, :] + 0.02 * rng.standard_normal((n_users, d)))
    noise = rng.standard_normal((n_items, d))
    noise -= np.outer(noise @ axis, axis)  # orthogonal to the axis
    noise = 0.05 * _unit(noise)
    t = np.linspace(0.1, 0.9, n_items)[:, None]
    items = (t * axis[None, :] + noise).astype(np.float32)
    return users, items


@pytest.mark.parametrize("n_items,k", [
    # 75 tiles (no list pre-pass): both lists ~ 300 of their 320 slots, past two first windows
    pytest.param(9_600, 31, id="lists-past-two-windows"),
    # the same construction over 1,250 blocks
    pytest.param(40_000, 31, id="40k"),
    # k = 1 lists hold 128 entries and every half-block is a record: the
    # appends overflow (acnt > m2) and the exact path takes the users
    pytest.param(9_600, 1, id="lists-past-m2"),
])
def test_list_mode_long_lists(ops, n_items, k):
    users, items = _rising(n_items, 70, n_items)
    _check(ops, users, items, k)


def test_both_modes_one_workspace(ops):
    """screen -> finish (lists), screen -> bound -> finish (the select's
    band), screen -> finish again (the next screen resets the mode): the
    same bits every time."""
    rng = np.random.default_rng(77)
    k = 31
    users = _unit(rng.standard_normal((301, 32)))
    users[11] = 0.0
    items = _unit(rng.standard_normal((20_000, 32)))
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    u = _dev(users)
    cat = ops.Catalog(_dev(items))
    ws = ops.ip_topk_workspace(len(users), cat, k, u.device)
    outs = []
    for with_bound in (False, True, False):
        s = torch.empty((len(users), k), dtype=torch.float32, device=u.device)
        r = torch.empty((len(users), k), dtype=torch.int32, device=u.device)
        e = torch.empty((len(users), k), dtype=torch.float64, device=u.device)
        ops.ip_topk_screen(u, cat, k, ws)
        if with_bound:
            b = ops.ip_topk_bound(u, cat, k, 4, ws)
            assert bool(torch.isfinite(b[users.any(1)]).all())
        ops.ip_topk_finish(u, cat, k, ws, s, r, out_exact=e)
        torch.cuda.synchronize()
        outs.append((s.cpu().numpy(), r.cpu().numpy(), e.cpu().numpy()))
    for s, r, e in outs:
        assert np.array_equal(r.astype(np.int64), ro)
        assert np.array_equal(s, so)
        assert np.array_equal(e, eo)


def test_list_mode_zero_user_and_padding(ops):
    rng = np.random.default_rng(3)
    users = _unit(rng.standard_normal((9, 32)))
    users[4] = 0.0
    _check(ops, users, _unit(rng.standard_normal((3_000, 32))), 31)
    _check(ops, users, _unit(rng.standard_normal((20, 32))), 31)  # n_items < k: padding rows


def test_list_mode_no_items(ops):
    users = _unit(np.random.default_rng(4).standard_normal((5, 32)))
    cat = ops.Catalog(torch.empty((0, 32), dtype=torch.float32, device="cuda"))
    s, r, e = ops.ip_topk(_dev(users), cat, 7, exact=True)
    torch.cuda.synchronize()
    assert bool((r == -1).all())
    assert bool((s == torch.finfo(torch.float32).min).all())
    assert bool((e == float("-inf")).all())


@pytest.mark.parametrize("d", [32, 128])
def test_list_mode_finish_without_packed_catalog(ops, d):
    """nrk_ip_topk_finish with catalog == NULL: no fp16 prefilter and no
    catalog header, the list cut compares in the scan's scaled units."""
    from nrk import _lib

    rng = np.random.default_rng(50 + d)
    k = 31
    users = _unit(rng.standard_normal((130, d)))
    items = _unit(rng.standard_normal((6_000, d)))
    so, ro, eo = oracle.ip_topk(users, items, k, exact=True)
    u = _dev(users)
    cat = ops.Catalog(_dev(items))
    ws = ops.ip_topk_workspace(len(users), cat, k, u.device)
    s = torch.empty((len(users), k), dtype=torch.float32, device=u.device)
    r = torch.empty((len(users), k), dtype=torch.int32, device=u.device)
    e = torch.empty((len(users), k), dtype=torch.float64, device=u.device)
    ops.ip_topk_screen(u, cat, k, ws)
    p = ops._ptr
    _lib.call("nrk_ip_topk_finish", p(u), len(users), p(cat.items), None, cat.n, cat.d, k, 0, p(s), p(r), p(e),
              p(ws), ws.numel(), ops._stream())
    torch.cuda.synchronize()
    assert np.array_equal(r.cpu().numpy().astype(np.int64), ro)
    assert np.array_equal(s.cpu().numpy(), so)
    assert np.array_equal(e.cpu().numpy(), eo)


def test_list_mode_heavy_duplicates(ops):
    """Four distinct item rows, 6,000 copies: the band overflows what the
    refine holds and the exact path answers (as in
    test_ip_topk_ties_overflow_fallback)."""
    rng = np.random.default_rng(9)
    base = _unit(rng.standard_normal((4, 32)))
    items = base[rng.integers(0, 4, size=6000)]
    users = _unit(rng.standard_normal((64, 32)))
    users[:8] = 0.0
    users[8:16] = base[rng.integers(0, 4, size=8)]
    _check(ops, users, items, 31)

"""nrk_ip_query's host side, no GPU: the workspace size and the plan are pure
functions, and every argument is refused before any device call (the pointers
handed in below are host addresses that no kernel ever sees)."""
import ctypes
import itertools
import types

import numpy as np
import pytest
import torch

from nrk import _lib, ops

MAXU = ops.IP_QUERY_MAX_USERS


def test_constants_match_the_header():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nrk.h")).read()
    assert int(re.search(r"#define NRK_IP_QUERY_MAX_USERS (\d+)", hdr).group(1)) == MAXU == 4096
    assert _lib.lib().nrk_abi_version() == 3  # the additions leave the ABI version alone


def test_workspace_bytes_positive_and_monotone():
    L = _lib.lib()
    users = [1, 7, 8, 9, 16, 17, 63, 64, 65, 512, 1000, 1024, 1025, 2048, 4095, MAXU]
    items = [1, 255, 256, 257, 3000, 131072, 131073, 364047, 5_000_000, 2 ** 30 - 1]
    dims = [1, 32, 50, 128, 256]
    ks = [1, 2, 31, 64, 128]
    f = L.nrk_ip_query_workspace_bytes
    for axis, (us, its, ds, kz) in enumerate([(users, [3000, 364047], [32], [31, 128]),
                                              ([1, 9, 64, MAXU], items, [32], [31, 128]),
                                              ([1, 64, MAXU], [3000, 364047], dims, [31]),
                                              ([1, 64, MAXU], [3000, 364047], [32], ks)]):
        grid = [us, its, ds, kz]
        others = [g for i, g in enumerate(grid) if i != axis]
        for fixed in itertools.product(*others):
            prev = 0
            for v in grid[axis]:
                args = list(fixed)
                args.insert(axis, v)
                b = f(*args)
                assert b > 0, args
                assert b >= prev, (axis, args, b, prev)
                prev = b
    # the largest call stays far below the exact path's n_users * n_items keys
    assert f(MAXU, 2 ** 30 - 1, 256, 128) < 64 << 20
    # outside the range there is no size
    for bad in ((MAXU + 1, 1000, 32, 31), (10, 1000, 32, 129), (10, 1000, 32, 0), (10, 1000, 0, 31),
                (10, 1000, 257, 31), (10, 2 ** 30, 32, 31), (-1, 1000, 32, 31)):
        assert f(*bad) == 0, bad


def test_workspace_holds_every_list_of_the_plan():
    """The size is a monotone bound, the plan's grid is not monotone in
    n_users: the bound must cover n_users * G lists of k 16-byte entries and
    their counts at every batch size."""
    L = _lib.lib()
    for n_items, k in ((1, 1), (3000, 31), (364047, 31), (364047, 128), (5_000_000, 128)):
        for n_users in list(range(1, 300)) + [511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, MAXU]:
            G = ops.ip_query_plan(n_users, n_items, 32, k)[2]
            assert L.nrk_ip_query_workspace_bytes(n_users, n_items, 32, k) >= n_users * G * (k * 16 + 4)


def test_plan_is_positive_and_pure():
    for args in ((1, 1, 32, 31), (1, 364047, 32, 31), (9, 600011, 32, 31), (4096, 364047, 32, 31),
                 (64, 5_000_000, 128, 128), (25, 100, 250, 1)):
        p = ops.ip_query_plan(*args)
        assert len(p) == 4 and all(isinstance(v, int) and v > 0 for v in p), (args, p)
        assert all(ops.ip_query_plan(*args) == p for _ in range(3))
        uq, rnd, G, cap = p
        assert rnd == 256 and cap >= args[3] + rnd  # a trimmed list takes one more round
        assert G <= -(-args[1] // rnd)  # never more workgroups than rounds
    # the catalog axis shrinks as user tiles fill the grid
    assert ops.ip_query_plan(1, 364047, 32, 31)[2] > ops.ip_query_plan(4096, 364047, 32, 31)[2]
    out = (ctypes.c_int32 * 4)()
    L = _lib.lib()
    assert L.nrk_ip_query_plan(1, 1000, 32, 31, None) == _lib.NRK_EINVAL and b"out is null" in L.nrk_last_error()
    assert L.nrk_ip_query_plan(1, 1000, 32, 129, ctypes.cast(out, _lib.P)) == _lib.NRK_EINVAL
    assert L.nrk_last_error()


def _host_call(n_users=4, n_items=1000, dim=32, k=31, users=True, items=True, out_s=True, out_r=True, ws=True,
               ws_bytes=None):
    """nrk_ip_query on host buffers: legal only for calls the checks refuse."""
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = lambda on: _lib.P(buf.ctypes.data) if on else None  # noqa: E731
    if ws_bytes is None:
        ws_bytes = L.nrk_ip_query_workspace_bytes(min(max(n_users, 0), MAXU), n_items, min(max(dim, 1), 256),
                                                  min(max(k, 1), 128))
    rc = L.nrk_ip_query(p(users), n_users, p(items), n_items, dim, k, 0, p(out_s), p(out_r), None, p(ws), ws_bytes,
                        None)
    return rc, L.nrk_last_error()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(k=129), _lib.NRK_EUNSUPPORTED, b"k > 128"),
    (dict(k=0), _lib.NRK_EINVAL, b"k must be"),
    (dict(dim=0), _lib.NRK_EINVAL, b"dim must be"),
    (dict(dim=257), _lib.NRK_EINVAL, b"dim must be"),
    (dict(n_users=MAXU + 1), _lib.NRK_EINVAL, b"n_users must be"),
    (dict(n_items=2 ** 30), _lib.NRK_EINVAL, b"n_items must be"),
    (dict(n_users=-1), _lib.NRK_EINVAL, b"negative"),
    (dict(users=False), _lib.NRK_EINVAL, b"null pointer"),
    (dict(ws=False), _lib.NRK_EINVAL, b"null pointer"),
    (dict(out_s=False), _lib.NRK_EINVAL, b"null output"),
    (dict(out_r=False), _lib.NRK_EINVAL, b"null output"),
    (dict(items=False), _lib.NRK_EINVAL, b"items null"),
    (dict(ws_bytes=255), _lib.NRK_EINVAL, b"workspace too small"),
])
def test_ip_query_refuses_before_any_device_work(kw, code, msg):
    rc, err = _host_call(**kw)
    assert rc == code
    assert msg in err and err.startswith(b"nrk_ip_query: ")
    with pytest.raises(NotImplementedError if code == _lib.NRK_EUNSUPPORTED else ValueError):
        _lib.check(rc, "nrk_ip_query")


def test_ip_query_short_workspace_is_one_byte_short():
    need = _lib.lib().nrk_ip_query_workspace_bytes(4, 1000, 32, 31)
    rc, err = _host_call(ws_bytes=need - 1)
    assert rc == _lib.NRK_EINVAL and b"workspace too small" in err


def test_ip_query_no_users_is_a_no_op():
    # nothing is read or written: null pointers pass
    rc, _ = _host_call(n_users=0, users=False, items=False, out_s=False, out_r=False, ws=False, ws_bytes=0)
    assert rc == _lib.NRK_OK


def _host_catalog(n=100, d=32):
    """What ip_query reads of an ops.Catalog, on the host (a Catalog itself
    needs a device)."""
    return types.SimpleNamespace(items=torch.zeros(n, d), n=n, d=d)


@pytest.mark.parametrize("k,msg", [(0, "k must be"), (129, "k must be"), (-3, "k must be")])
def test_ops_ip_query_k_range(k, msg):
    with pytest.raises(ValueError, match=msg):
        ops.ip_query(torch.zeros(4, 32), _host_catalog(), k)


def test_ops_ip_query_argument_errors():
    cat = _host_catalog()
    with pytest.raises(ValueError, match=r"users must be \[n, 32\]"):
        ops.ip_query(torch.zeros(4, 16), cat, 31)  # dim mismatch
    with pytest.raises(ValueError, match=r"users must be \[n, 32\]"):
        ops.ip_query(torch.zeros(32), cat, 31)
    with pytest.raises(ValueError, match="expected torch.float32"):
        ops.ip_query(torch.zeros(4, 32, dtype=torch.float64), cat, 31)
    with pytest.raises(ValueError, match="n_users must be"):
        ops.ip_query(torch.zeros(MAXU + 1, 32), cat, 31)
    with pytest.raises(ValueError, match="dim must be"):
        ops.ip_query(torch.zeros(4, 257), _host_catalog(d=257), 31)
    for bad in (float("nan"), float("inf"), -float("inf")):
        u = torch.zeros(4, 32)
        u[2, 7] = bad
        with pytest.raises(ValueError, match="users must be finite"):
            ops.ip_query(u, cat, 31)
        # not asked to look: the next check (host tensors) is what stops the call
        with pytest.raises(ValueError, match="device"):
            ops.ip_query(u, cat, 31, check_finite=False)
    with pytest.raises(ValueError, match="device"):
        ops.ip_query(torch.zeros(4, 32), cat, 31)


def test_ops_plan_and_workspace_argument_errors():
    for bad in ((1, 1000, 32, 129), (1, 1000, 32, 0), (1, 1000, 0, 31), (1, 1000, 257, 31), (MAXU + 1, 1000, 32, 31),
                (1, 2 ** 30, 32, 31)):
        with pytest.raises(ValueError):
            ops.ip_query_plan(*bad)
    with pytest.raises(ValueError, match="k must be"):
        ops.ip_query_workspace(4, _host_catalog(), 129, "cpu")
    with pytest.raises(ValueError, match="n_users must be"):
        ops.ip_query_workspace(MAXU + 1, _host_catalog(), 31, "cpu")
    ws = ops.ip_query_workspace(4, _host_catalog(), 31, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == _lib.lib().nrk_ip_query_workspace_bytes(4, 100, 32, 31)


def test_recaller_query_max_users_is_a_class_default():
    from nrk.recall.youtubednn_recaller import YoutubeDNNRecaller

    assert isinstance(YoutubeDNNRecaller.query_max_users, int)
    assert 0 <= YoutubeDNNRecaller.query_max_users <= MAXU
    rec = YoutubeDNNRecaller(device="cpu")
    rec.query_max_users = 0
    assert "query_max_users" in vars(rec) and "query_max_users" not in vars(YoutubeDNNRecaller(device="cpu"))

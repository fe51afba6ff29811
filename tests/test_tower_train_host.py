"""YouTubeDNN training, the parts that need no GPU: the plain-torch
restatement (tests/tower_train_restated.py) against the fixture made by
executing the reference (tests/golden/make_golden_ytdnn_train.py), the
argument checks of every new C ABI entry, the workspace query and the new
config fields."""
import ctypes

import numpy as np
import pytest
import torch

import tower_train_restated as R
from nrk import _lib
from nrk.config import RecallConfig

FP32_EPS = float(np.finfo(np.float32).eps)


def test_restatement_matches_the_reference_fixture(golden):
    """Two pins.  The fp32 restatement runs the reference's own torch
    operators, so it reproduces the fixture (measured: bit for bit; asserted
    to twice the fixture's own distance from fp64, which leaves room for
    another thread count's summation order).  The fp64 restatement differs
    from the fixture by fp32 rounding only: within 64 eps32 of the tensor's
    largest magnitude for gradients and losses (a few hundred roundings along
    any path of a 2-layer, T = 30 model; a wrong formula is off by O(1)), and
    within 1 % of the 7 lr any parameter can move in 7 Adam steps for the
    final state."""
    g = golden("ytdnn_train_small")
    off, items, init, batches, T = R.fixture_parts(g)
    assert len(batches) == 7 and len(batches[-1][0]) == 37 and int(g["s_pos"].max()) > T
    loss32, g32 = R.grads(init, off, items, batches[0], T, torch.float32)
    loss64, g64 = R.grads(init, off, items, batches[0], T, torch.float64)
    for k in g32:
        e_ref = R.err(g["grad." + k], g64[k])
        scale = float(np.abs(g64[k]).max())
        print(f"grad {k}: fixture-vs-fp64 {e_ref:.3e}, restated32-vs-fixture {R.err(g32[k], g['grad.' + k]):.3e}, "
              f"max |g| {scale:.3e}")
        assert e_ref <= 64 * FP32_EPS * scale
        assert R.err(g32[k], g["grad." + k]) <= 2 * e_ref
    l32, f32 = R.train(init, off, items, batches, T, torch.float32, lr=float(g["lr"]))
    l64, f64 = R.train(init, off, items, batches, T, torch.float64, lr=float(g["lr"]))
    e_ref = R.err(g["losses"], l64)
    print(f"losses: fixture-vs-fp64 {e_ref:.3e}, restated32-vs-fixture {R.err(l32, g['losses']):.3e}")
    assert e_ref <= 64 * FP32_EPS and R.err(l32, g["losses"]) <= 2 * e_ref
    assert abs(loss32 - g["losses"][0]) <= 2 * e_ref and abs(loss64 - l64[0]) == 0
    for k in f32:
        e_ref = R.err(g["final." + k], f64[k])
        print(f"final {k}: fixture-vs-fp64 {e_ref:.3e}, restated32-vs-fixture {R.err(f32[k], g['final.' + k]):.3e}")
        # 7 steps of at most lr each bound any parameter's movement; two runs of the same signs agree far closer
        assert e_ref <= 7 * float(g["lr"]) * 1e-2
        assert R.err(f32[k], g["final." + k]) <= 2 * e_ref


def test_restated_split_rule_matches_prepare_data(golden):
    g = golden("ytdnn_train_small")
    off, items = R.csr_from_clicks(g["click_user"], g["click_item"], g["click_ts"])
    pos = R.positives(off)
    triples = np.column_stack([pos[:, 0], pos[:, 1], items[off[pos[:, 0]] + pos[:, 1]]])
    assert np.array_equal(triples[np.lexsort(triples.T[::-1])], g["positives"])


def test_config_carries_the_training_fields():
    c = RecallConfig()
    assert (c.youtubednn_negsample, c.youtubednn_epochs, c.youtubednn_batch_size, c.youtubednn_learning_rate) == \
        (4, 1, 256, 0.001)


def _widths(*w):
    return ctypes.cast((ctypes.c_int * len(w))(*w), _lib.P), len(w)


def test_workspace_query():
    L = _lib.lib()
    w, n = _widths(64, 32)
    small = L.nrk_tt_train_workspace_bytes(250000, 364047, 32, n, w, 30, 256)
    large = L.nrk_tt_train_workspace_bytes(250000, 364047, 32, n, w, 30, 4096)
    assert 0 < small < large < 1 << 30
    w1, n1 = _widths(16)
    assert L.nrk_tt_train_workspace_bytes(10, 10, 16, n1, w1, 1, 1) > 0
    assert L.nrk_tt_train_workspace_bytes(10, 10, 24, n1, w1, 30, 64) == 0 and b"dim must be" in L.nrk_last_error()


def test_train_grad_argument_errors():
    L = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: every call below fails its checks first

    def grad(dim=32, widths=(64, 32), batch=64, seq_len=30, p=0.2, ptr=one, ws_bytes=1 << 30, step=0):
        w, n = _widths(*widths)
        return L.nrk_tt_train_grad(ptr, 100, ptr, 100, dim, ptr, n, w, ptr, ptr, ptr, ptr, ptr, ptr, batch, seq_len,
                                   p, 7, step, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ws_bytes, None)

    assert grad(ptr=None) == _lib.NRK_EINVAL and b"null pointer" in L.nrk_last_error()
    with pytest.raises(ValueError):
        _lib.check(grad(ptr=None), "nrk_tt_train_grad")
    assert grad(dim=24, widths=(64, 24)) == _lib.NRK_EUNSUPPORTED and b"dim must be" in L.nrk_last_error()
    assert grad(widths=(300, 32)) == _lib.NRK_EUNSUPPORTED and b"widths" in L.nrk_last_error()
    assert grad(widths=(64, 16)) == _lib.NRK_EINVAL and b"last hidden width" in L.nrk_last_error()
    assert grad(widths=(32,) * 9) == _lib.NRK_EUNSUPPORTED
    for batch in (0, 8193):
        assert grad(batch=batch) == _lib.NRK_EINVAL and b"batch must be" in L.nrk_last_error()
    for seq_len in (0, 65):
        assert grad(seq_len=seq_len) == _lib.NRK_EINVAL and b"seq_len" in L.nrk_last_error()
    for p in (1.0, -0.1, 1.5):
        assert grad(p=p) == _lib.NRK_EINVAL and b"dropout p" in L.nrk_last_error()
    assert grad(step=-1) == _lib.NRK_EINVAL
    assert grad(ws_bytes=16) == _lib.NRK_EINVAL and b"workspace too small" in L.nrk_last_error()


def test_dropout_mask_argument_errors():
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    assert L.nrk_tt_dropout_mask(1, 0, 0, 64, 64, 0.2, None, None) == _lib.NRK_EINVAL
    assert b"null pointer" in L.nrk_last_error()
    for batch in (0, 8193):
        assert L.nrk_tt_dropout_mask(1, 0, 0, batch, 64, 0.2, one, None) == _lib.NRK_EINVAL
    assert L.nrk_tt_dropout_mask(1, 0, 0, 64, 300, 0.2, one, None) == _lib.NRK_EINVAL
    assert L.nrk_tt_dropout_mask(1, 0, 8, 64, 64, 0.2, one, None) == _lib.NRK_EINVAL
    for p in (1.0, -0.5):
        assert L.nrk_tt_dropout_mask(1, 0, 0, 64, 64, p, one, None) == _lib.NRK_EINVAL
        assert b"dropout p" in L.nrk_last_error()


def test_adam_step_argument_errors():
    L = _lib.lib()
    one = ctypes.c_void_p(16)

    def adam(ptr=one, dim=32, t=1, lr=1e-3, n_w=100):
        return L.nrk_tt_adam_step(ptr, ptr, ptr, ptr, n_w, ptr, ptr, ptr, 10, ptr, ptr, ptr, ptr, ptr, ptr, 10, ptr,
                                  ptr, ptr, dim, lr, 0.9, 0.999, 1e-8, t, None)

    assert adam(ptr=None) == _lib.NRK_EINVAL and b"null pointer" in L.nrk_last_error()
    assert adam(dim=24) == _lib.NRK_EUNSUPPORTED
    assert adam(dim=24) == _lib.NRK_EUNSUPPORTED and b"dim must be" in L.nrk_last_error()
    assert adam(t=0) == _lib.NRK_EINVAL and b"1-based" in L.nrk_last_error()
    assert adam(lr=0.0) == _lib.NRK_EINVAL
    assert adam(n_w=0) == _lib.NRK_EINVAL


def test_make_samples_argument_errors():
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    assert L.nrk_tt_make_samples_count(None, 10, None, None) == _lib.NRK_EINVAL
    assert b"null pointer" in L.nrk_last_error()
    assert L.nrk_tt_make_samples_count(one, 0, one, None) == _lib.NRK_EINVAL
    assert L.nrk_tt_make_samples(None, None, 10, None, 5, 0, None, 0, 1, None, None, None, None, None) == \
        _lib.NRK_EINVAL
    assert b"null pointer" in L.nrk_last_error()
    assert L.nrk_tt_make_samples(one, one, 10, one, 5, 4, None, 0, 1, one, one, one, one, None) == _lib.NRK_EINVAL
    assert b"pool" in L.nrk_last_error()
    assert L.nrk_tt_make_samples(one, one, 10, one, 5, -1, None, 0, 1, one, one, one, one, None) == _lib.NRK_EINVAL
    # no positives: nothing to write, nothing dereferenced
    assert L.nrk_tt_make_samples(None, None, 10, None, 0, 0, None, 0, 1, None, None, None, None, None) == _lib.NRK_OK

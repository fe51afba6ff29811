"""DIN training for 1 to 4 MLP hidden layers and either activation, the parts
that need no GPU: the plain-torch restatement (tests/din_train_layers_restated.py)
against the fixture made by executing the reference, DINRanker's initial state
and artifacts, the argument refusals and the packed layout of the new C entry
points, and what tests/test_gpu_din_train_layers.py presumes of its inputs."""
import ctypes
import os

import numpy as np
import pytest
import torch

import din_train_layers_cases as C
import din_train_layers_restated as RL
import din_train_restated as R
from nrk import _lib
from nrk.config import RankConfig
from nrk.rank.din import DINRanker, _expected_state

MODELS = list(RL.MODELS)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("din_train_small"), golden("din_train_layers_small")


def _same(what, a, b):
    """Exact agreement is expected (the same torch ops on the same machine
    type); otherwise rtol 1e-6.  Prints which one held."""
    a, b = np.asarray(a), np.asarray(b)
    if np.array_equal(a, b):
        print(f"{what}: exact")
        return
    print(f"{what}: not exact, max |diff| {np.max(np.abs(a - b)):.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 * float(np.max(np.abs(b))))


def test_two_dice_layers_are_din_train_restated(fx):
    """On the model din_train_restated states, this restatement is the same
    torch operations: bit-equal loss and gradients."""
    torch.set_num_threads(1)
    init, feats, batches, _ = R.fixture_parts(fx[0])
    assert RL.state_keys(feats) == R.state_keys(feats)
    assert RL.state_keys(feats, alphas=False) == R.state_keys(feats, alphas=False)
    for dt in (torch.float32, torch.float64):
        a, b = R.grads(init, feats, batches[0], dt), RL.grads(init, feats, batches[0], dt)
        assert a[0] == b[0] and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    rng = np.random.default_rng(1)
    st, fs = RL.random_state(rng, C.vocabs_for(2), (40, 24))
    st0, _ = R.random_state(np.random.default_rng(1), C.vocabs_for(2), (40, 24))
    assert list(st) == list(st0) and all(np.array_equal(st[k], st0[k]) for k in st)


@pytest.mark.parametrize("model", MODELS)
def test_restatement_matches_the_reference_run(fx, model):
    torch.set_num_threads(1)
    g = fx[1]
    init, feats, batches, lr = RL.fixture_parts(*fx, model)
    hidden, act = RL.MODELS[model]
    assert RL.mlp_shape(init) == (list(hidden), act)
    _, g32 = RL.grads(init, feats, batches[0], torch.float32)
    pre = f"{model}.grad."
    assert sorted(pre + k for k in g32) == sorted(k for k in g.files if k.startswith(pre))
    for k in g32:
        _same("grad " + k, g32[k], g[pre + k])
    gaps = [] if act == "prelu" else None
    losses, final = RL.train(init, feats, batches, torch.float32, lr=lr, gaps=gaps)
    _same("losses", losses, g[f"{model}.losses"])
    pre = f"{model}.final."
    assert list(final) == RL.state_keys(feats, len(hidden), act) == [k[len(pre):] for k in g.files
                                                                      if k.startswith(pre)]
    for k in final:
        _same("final " + k, final[k], g[pre + k])
        if k.endswith(".alpha"):
            assert np.array_equal(final[k], init[k])
    if act == "prelu":
        # the kink condition over the 7 steps of the run the GPU test repeats
        zmin, ez = min(gaps, key=lambda x: x[0] / x[1])
        print(f"{model}: smallest gap min |z| {zmin:.3e}, e_z {ez:.3e}, ratio {zmin / ez:.1f}; fixture "
              f"{g[model + '.prelu_gap']}")
        assert zmin >= C.KINK * ez
        _same("prelu_gap", [zmin, ez], g[f"{model}.prelu_gap"])
        for k in RL.slope_keys(init):
            assert np.array_equal(init[k], np.array([0.25], np.float32)) and final[k][0] != 0.25


def _ranker(tmp_path, **kw):
    return DINRanker(RankConfig(_project_root=str(tmp_path), **kw), device="cpu")


@pytest.mark.parametrize("model", MODELS)
def test_init_state_is_the_reference_initialisation(fx, tmp_path, model):
    """_init_state under the fixture's seed draws what DINModel(...) drew:
    slopes 0.25, alphas = widths, DINModel's key order."""
    init, feats, _, _ = RL.fixture_parts(*fx, model)
    hidden, act = RL.MODELS[model]
    vocabs = [{f: init[f"{grp}.{f}.weight"].shape[0] for f in fs} for grp, fs in zip(R.GROUPS, feats)]
    rk = _ranker(tmp_path, random_seed=int(fx[1][f"{model}.seed"]), din_activation=act,
                 din_mlp_hidden_units=list(hidden))
    sd = rk._init_state(*vocabs)
    assert list(sd) == list(_expected_state(*vocabs, 32, list(hidden), act)) == RL.state_keys(feats, len(hidden), act)
    for k in sd:
        assert np.array_equal(sd[k].numpy(), init[k]), k
    for n, unit in enumerate(hidden):
        if act == "prelu":
            assert sd[f"mlp.{2 * n + 1}.weight"].tolist() == [0.25]
        else:
            assert float(sd[f"mlp.{2 * n + 1}.alpha"]) == unit


class _HostTrainer:
    """Stands in for ops.DinTrainParams where there is no device."""

    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return {k: torch.as_tensor(np.asarray(v)).clone() for k, v in self.sd.items()}


@pytest.mark.parametrize("model", ["prelu_24x10", "dice_20x12x6"])
def test_save_model_artifacts_pass_load_model_checks(fx, tmp_path, model):
    """din_model.pth and din_model_metadata.pkl of a PReLU and of a 3-layer
    model: key order and shapes are _expected_state's for the metadata's
    activation and widths, which is what load_model checks."""
    from nrk.rank.base import load_pickle

    init, feats, _, _ = RL.fixture_parts(*fx, model)
    hidden, act = RL.MODELS[model]
    rk = _ranker(tmp_path, din_activation=act, din_mlp_hidden_units=list(hidden))
    rk.user_profile_features, rk.item_features, rk.context_features = feats
    rk.trainer = _HostTrainer(init)
    out = tmp_path / "model"
    rk.save_model(str(out))
    meta = load_pickle(os.path.join(out, "din_model_metadata.pkl"))
    assert meta["din_activation"] == act and meta["din_mlp_hidden_units"] == list(hidden)
    rk._check_model_config(meta["din_activation"], meta["din_mlp_hidden_units"])
    sd = torch.load(os.path.join(out, "din_model.pth"), map_location="cpu", weights_only=True)
    vocabs = [{f: init[f"{grp}.{f}.weight"].shape[0] for f in fs} for grp, fs in zip(R.GROUPS, feats)]
    exp = _expected_state(*vocabs, meta["din_embedding_dim"], meta["din_mlp_hidden_units"], meta["din_activation"])
    assert list(sd) == list(exp) and all(tuple(sd[k].shape) == exp[k] for k in exp)
    assert all(np.array_equal(sd[k].numpy(), init[k]) for k in exp)


def test_train_config_is_range_checked():
    for act, hidden in (("relu", [24, 10]), ("prelu", [8] * 5), ("dice", []), ("prelu", [24, 1025]), ("dice", [0])):
        with pytest.raises(NotImplementedError):
            DINRanker._check_model_config(act, hidden)
    for act, hidden in (("prelu", [1]), ("dice", [1024, 1, 7, 3])):
        DINRanker._check_model_config(act, hidden)


def _widths(ws):
    return None if ws is None else (ctypes.c_int32 * max(1, len(ws)))(*ws)


def test_mlp_entry_points_refuse_unsupported_shapes():
    """Before any pointer is touched: an error code and a zero workspace."""
    L = _lib.lib()
    ok = dict(rows=500, dim=32, dtype=0, nu=5, ni=4, nc=16, nl=2, w=(200, 80), act=1, B=256, T=50)

    def ws_bytes(a):
        return L.nrk_din_train_mlp_workspace_bytes(a["rows"], a["dim"], a["dtype"], a["nu"], a["ni"], a["nc"],
                                                   a["nl"], _widths(a["w"]), a["act"], a["B"], a["T"])

    def grad_rc(a):
        return L.nrk_din_train_grad_mlp(None, a["rows"], a["dim"], a["dtype"], None, a["nu"], a["ni"], a["nc"], None,
                                        a["nl"], _widths(a["w"]), a["act"], None, None, None, None, None, None,
                                        a["B"], a["T"], None, None, None, None, None, None, 0, None)

    assert ws_bytes(ok) > 0
    assert grad_rc(ok) == _lib.NRK_EINVAL and b"null pointer" in L.nrk_last_error()
    U, E = _lib.NRK_EUNSUPPORTED, _lib.NRK_EINVAL
    for change, word, rc in ((dict(nl=0, w=()), b"n_layers", U), (dict(nl=5, w=(8,) * 5), b"n_layers", U),
                             (dict(w=(200, 0)), b"widths", U), (dict(w=(1025, 80)), b"widths", U),
                             (dict(act=2), b"activation", E), (dict(w=None), b"widths", E),
                             (dict(dim=64), b"din_embedding_dim", U), (dict(B=1), b"batch", U),
                             (dict(T=129), b"seq_len", U), (dict(dtype=1), b"fp32", U), (dict(ni=3), b"n_item", U)):
        a = {**ok, **change}
        assert ws_bytes(a) == 0, change
        assert word in L.nrk_last_error(), (change, L.nrk_last_error())
        assert grad_rc(a) == rc, change
        assert word in L.nrk_last_error(), (change, L.nrk_last_error())
    for act in (0, 1):
        for nl in (1, 2, 3, 4):
            a = {**ok, "act": act, "nl": nl, "w": (24, 16, 12, 8)[:nl]}
            assert ws_bytes(a) > 0 and grad_rc(a) == E and b"null pointer" in L.nrk_last_error()
    # two Dice layers: the workspace of the entry point they have always had
    a = {**ok, "act": 0}
    assert ws_bytes(a) == L.nrk_din_train_workspace_bytes(500, 32, 0, 5, 4, 16, 200, 80, 0, 256, 50)


@pytest.mark.parametrize("act", ["dice", "prelu"])
@pytest.mark.parametrize("hidden", [(40,), (200, 80), (64, 65, 8), (24, 16, 12, 8)])
def test_n_weights_matches_the_packed_layout(hidden, act):
    from nrk import ops

    L = _lib.lib()
    nu, ni, nc = 5, 4, 16
    n = L.nrk_din_train_mlp_n_weights(32, nu, ni, nc, len(hidden), _widths(hidden), ops.DIN_ACTIVATIONS.index(act))
    vocabs = ({f"u{i}": 3 for i in range(nu)}, {f"i{i}": 3 for i in range(ni)}, {f"c{i}": 3 for i in range(nc)})
    state, feats = RL.random_state(np.random.default_rng(0), vocabs, hidden, act)
    _, w_keys, alphas, order = ops.din_state_keys(*feats, hidden, act)
    assert n == sum(np.size(state[k]) for k in w_keys)
    assert order == RL.state_keys(feats, len(hidden), act) and sorted(w_keys + alphas) == sorted(
        k for k in order if "embedding_dict" not in k)
    if act == "prelu":  # each slope right after its layer's bias
        assert all(w_keys[w_keys.index(f"mlp.{2 * i}.bias") + 1] == f"mlp.{2 * i + 1}.weight"
                   for i in range(len(hidden)))
    assert L.nrk_din_train_mlp_n_weights(32, nu, ni, nc, 5, _widths((8,) * 5), 0) == 0
    assert b"n_layers" in L.nrk_last_error()
    if (tuple(hidden), act) == ((200, 80), "dice"):
        assert ops.din_state_keys(*feats) == ops.din_state_keys(*feats, hidden, act)


# ------------------------------------------- what the GPU cases presume --
@pytest.mark.parametrize("case", C.grad_cases(), ids=lambda c: c["id"])
def test_gpu_case_inputs(case):
    """No Dice column of std 0, and for a PReLU case the kink condition on
    every batch; (e_ref > 0 for every compared tensor is asserted where it is
    computed, in the GPU test, before the kernel's figure is looked at)."""
    state, feats, batches = C.build(case)
    assert RL.mlp_shape(state) == (list(case["hidden"]), case["act"])
    sd = min(RL.min_dice_std(state, feats, b) for b in batches)
    assert sd > 0, f"Dice std 0 in {case['id']}"
    if case["act"] == "prelu":
        ratio = C.kink_ratio(state, feats, batches)
        print(f"{case['id']}: min |z| / e_z = {ratio:.1f}, min Dice std {sd:.3e}")
        assert ratio >= C.KINK
        # per batch: beyond about 1.5e5 elements no draw of a few dozen meets the condition
        assert max(case["Bs"]) * sum(case["hidden"]) <= 1.5e5


def test_loss_only_case_inputs():
    """Too large for the kink condition, hence losses only; its Dice columns
    (the attention's) have no std of 0 either."""
    c = C.loss_only_case()
    assert not c["grads"] and c["Bs"][0] * sum(c["hidden"]) > 1e6
    state, feats, batches = C.build(c)
    sd = min(RL.min_dice_std(state, feats, b) for b in batches)
    print(f"{c['id']}: min Dice std {sd:.3e}")
    assert sd > 0

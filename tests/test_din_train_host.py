"""DIN training, the parts that need no GPU: the plain-torch restatement
(tests/din_train_restated.py) against the fixture made by executing the
reference, the host ETL and artifacts of DINRanker.train, and the argument
refusals of the C entry points."""
import os

import numpy as np
import pytest
import torch

import din_train_restated as R
from nrk import _lib
from nrk.config import RankConfig
from nrk.rank.din import DINRanker, _expected_state


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("din_train_small")
    return g, R.fixture_parts(g)


def _same(what, a, b):
    """Exact agreement is expected (the same torch ops on the same machine
    type); otherwise rtol 1e-6.  Prints which one held."""
    a, b = np.asarray(a), np.asarray(b)
    if np.array_equal(a, b):
        print(f"{what}: exact")
        return
    print(f"{what}: not exact, max |diff| {np.max(np.abs(a - b)):.3e}")
    np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 * float(np.max(np.abs(b))))


def test_restatement_matches_the_reference_run(fx):
    torch.set_num_threads(1)
    g, (init, feats, batches, lr) = fx
    assert [len(b["label"]) for b in batches] == [64] * 6 + [37]
    assert (np.concatenate([b["mask"] for b in batches]).sum(1) == 0).mean() > 0.15
    _, g32 = R.grads(init, feats, batches[0], torch.float32)
    assert sorted("grad." + k for k in g32) == sorted(k for k in g.files if k.startswith("grad."))
    for k in g32:
        _same("grad " + k, g32[k], g["grad." + k])
    losses, final = R.train(init, feats, batches, torch.float32, lr=lr)
    _same("losses", losses, g["losses"])
    assert list(final) == R.state_keys(feats) == [k[len("final."):] for k in g.files if k.startswith("final.")]
    for k in final:
        _same("final " + k, final[k], g["final." + k])
        if k.endswith(".alpha"):
            assert np.array_equal(final[k], g["init." + k])


def test_pad_rows_and_masked_positions_carry_gradient(fx):
    """What a backward that skips masked positions would miss."""
    g, (init, feats, batches, _) = fx
    for f in feats[1]:
        assert np.abs(g[f"grad.item_embedding_dict.{f}.weight"][0]).max() > 0


def _ranker(tmp_path, **kw):
    return DINRanker(RankConfig(_project_root=str(tmp_path), **kw), device="cpu")


def test_negative_sampling_equals_the_reference_frame(fx, tmp_path):
    import pandas as pd

    g, _ = fx
    rk = _ranker(tmp_path, random_seed=int(g["ns_seed"]))
    frame = pd.DataFrame({"row": np.arange(len(g["ns_label"])), "label": g["ns_label"]})
    out = rk._apply_negative_sampling(frame, ratio=float(g["ns_ratio"]))
    assert np.array_equal(out["row"].to_numpy(), g["ns_rows"])
    assert list(out.index) == list(range(len(out)))
    # nothing to drop: the frame comes back as it is
    assert rk._apply_negative_sampling(frame, ratio=1000.0) is frame


def test_init_state_is_the_reference_initialisation(fx, tmp_path):
    """_init_state under the fixture's seed draws what DINModel(...) drew."""
    g, (init, feats, _, _) = fx
    vocabs = [{f: init[f"{grp}.{f}.weight"].shape[0] for f in fs} for grp, fs in zip(R.GROUPS, feats)]
    sd = _ranker(tmp_path, random_seed=23)._init_state(*vocabs)
    assert list(sd) == R.state_keys(feats)
    for k in sd:
        assert np.array_equal(sd[k].numpy(), init[k]), k


class _HostTrainer:
    """Stands in for ops.DinTrainParams where there is no device."""

    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return {k: torch.as_tensor(np.asarray(v)).clone() for k, v in self.sd.items()}


def test_save_model_artifacts_pass_load_model_checks(fx, tmp_path):
    """din_model.pth / din_model_metadata.pkl / label_encoders.pkl as the
    reference writes them (DIN.py:1285-1326): key order and shapes are
    _expected_state's, and the files read back as load_model reads them."""
    from nrk.rank.base import load_pickle

    g, (init, feats, _, _) = fx
    rk = _ranker(tmp_path)
    rk.user_profile_features, rk.item_features, rk.context_features = feats
    rk.label_encoders = {"some_feature": "encoder"}
    with pytest.raises(ValueError):
        rk.save_model()
    rk.trainer = _HostTrainer(init)
    out = tmp_path / "model"
    rk.save_model(str(out))
    sd = torch.load(os.path.join(out, "din_model.pth"), map_location="cpu", weights_only=True)
    vocabs = [{f: init[f"{grp}.{f}.weight"].shape[0] for f in fs} for grp, fs in zip(R.GROUPS, feats)]
    exp = _expected_state(*vocabs, 32, [200, 80])
    assert list(sd) == list(exp) and all(tuple(sd[k].shape) == exp[k] for k in exp)
    assert all(np.array_equal(sd[k].numpy(), init[k]) for k in exp)
    meta = load_pickle(os.path.join(out, "din_model_metadata.pkl"))
    assert meta == {"user_profile_features": feats[0], "item_features": feats[1], "context_features": feats[2],
                    "din_embedding_dim": 32, "din_attention_hidden_units": [36], "din_mlp_hidden_units": [200, 80],
                    "din_activation": "dice", "din_seq_max_len": rk.config.din_seq_max_len}
    assert load_pickle(os.path.join(out, "label_encoders.pkl")) == rk.label_encoders


def test_training_entry_points_refuse_unsupported_shapes():
    """Before any pointer is touched: NRK_EUNSUPPORTED and a zero workspace."""
    L = _lib.lib()
    ok = dict(rows=500, dim=32, dtype=0, nu=5, ni=4, nc=16, h1=200, h2=80, act=0, B=256, T=50)
    assert L.nrk_din_train_workspace_bytes(*ok.values()) > 0

    def grad_rc(a):
        return L.nrk_din_train_grad(None, a["rows"], a["dim"], a["dtype"], None, a["nu"], a["ni"], a["nc"], None,
                                    a["h1"], a["h2"], a["act"], None, None, None, None, None, None, a["B"], a["T"],
                                    None, None, None, None, None, None, 0, None)

    assert grad_rc(ok) == _lib.NRK_EINVAL and b"null pointer" in L.nrk_last_error()
    for change, word in ((dict(dim=64), b"din_embedding_dim"), (dict(ni=3), b"n_item"), (dict(B=1), b"batch"),
                         (dict(dtype=1), b"fp32"), (dict(act=1), b"Dice"), (dict(T=129), b"seq_len")):
        a = {**ok, **change}
        assert L.nrk_din_train_workspace_bytes(*a.values()) == 0, change
        assert word in L.nrk_last_error(), (change, L.nrk_last_error())
        assert grad_rc(a) == _lib.NRK_EUNSUPPORTED, change
        with pytest.raises(NotImplementedError):
            _lib.check(grad_rc(a), "nrk_din_train_grad")
    assert L.nrk_din_adam_step(None, None, None, None, 10, None, None, None, 10, 64, None, None, None, 1e-3, 0.9,
                               0.999, 1e-8, 1, None) == _lib.NRK_EUNSUPPORTED
    assert L.nrk_din_adam_step(None, None, None, None, 10, None, None, None, 10, 32, None, None, None, 1e-3, 0.9,
                               0.999, 1e-8, 0, None) == _lib.NRK_EINVAL

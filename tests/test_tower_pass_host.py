"""CPU side of tests/test_gpu_tower_pass.py: nrk_tt_user_pass_users through the
C ABI (no launch), and the GPU file's cases (imported, so they cannot drift)
held to what tests/test_tower_host.py requires of its own: ids in range,
padded slots in range and never the masked index 0, the lengths each case
claims, and, for the rows compared with the fp64 reference (a case of
tests/test_gpu_tower_shapes.py, conditioned by its make_case), that file's
own checks by import: the bar met by the fp32 oracle and a one-slot error
seen at more than 10 bars.
"""

import numpy as np
import pytest

import test_gpu_tower_pass as P
import test_gpu_tower_shapes as S
import test_tower_host as H
from oracle import oracle

G = P.G_NOMINAL


@pytest.fixture(scope="module")
def L():
    from nrk import _lib

    return _lib.lib()


def test_query_values_for_every_supported_shape(L):
    assert L.nrk_abi_version() == 3  # the addition leaves the ABI version alone
    for dim in (16, 32, 64):
        for h0 in range(1, 129):
            assert L.nrk_tt_user_pass_users(dim, h0) == (G if h0 <= 64 else 0), (dim, h0)
            assert L.nrk_last_error() == b"", (dim, h0)  # 0 is an answer there, not an error


@pytest.mark.parametrize("dim,h0,what", [(8, 64, b"dim"), (0, 64, b"dim"), (48, 64, b"dim"), (128, 64, b"dim"),
                                         (-32, 64, b"dim"), (32, 0, b"h0"), (32, -1, b"h0"), (32, 129, b"h0"),
                                         (64, 1 << 20, b"h0")])
def test_query_rejects(L, dim, h0, what):
    assert L.nrk_tt_user_pass_users(dim, h0) == 0
    err = L.nrk_last_error()
    assert err.startswith(b"nrk_tt_user_pass_users: ") and what in err, err
    from nrk import ops

    with pytest.raises(ValueError, match=what.decode()):
        ops.tt_user_pass_users(dim, h0)
    assert ops.tt_user_pass_users(32, 64) == G and L.nrk_last_error() == b""  # the error does not stick


def _in_range(k, hlen=None):
    hlen = k["hlen"] if hlen is None else hlen
    T = k["T"]
    assert k["hist"].shape == (k["n"], T) and hlen.shape == (k["n"],)
    assert hlen.min() >= 0 and hlen.max() <= T
    assert k["hist"].min() > 0 and k["hist"].max() < S.I_ROWS  # padded slots too: in range, never 0
    assert k["uid"].min() >= 0 and k["uid"].max() < S.U_ROWS


def test_tail_and_position_cases():
    k = P.tail_inputs(G)
    _in_range(k)
    assert k["n"] == 2 * G + 1 and (k["D"], k["h0"], k["T"]) == (32, 64, 30)
    assert np.array_equal(k["hlen"], np.arange(2 * G + 1))  # an empty history first, then growing
    k = P.position_inputs(G)
    _in_range(k)
    assert k["n"] == 4 * G and (k["D"], k["h0"], k["T"]) == (32, 64, 30)
    assert (k["hlen"] == 0).any() and (k["hlen"] > 0).sum() >= G and len(np.unique(k["hlen"])) > 3  # mixed
    # a gather round is 4 loads of 2 phases: 9 and 17 leave one slot for the next round
    assert set(P.POS_LENS) >= {0, 1, k["T"]} and sum(L_ % 8 == 1 and L_ > 1 for L_ in P.POS_LENS) == 2
    assert P.POS_PASSES == (0, 1, k["n"] // G - 1)  # the first pass, a middle one and the last
    for pas in P.POS_PASSES:
        for pos in range(G):
            for length in P.POS_LENS:
                hlen = P.position_lens(k, G, pas, pos, length)
                _in_range(k, hlen)
                changed = np.flatnonzero(hlen != k["hlen"])
                assert hlen[pas * G + pos] == length and set(changed) <= {pas * G + pos}


def test_boundary_cases():
    assert sorted(h for D, h in P.BOUNDARY if D == 32) == [1, 3, 60, 63, 64, 65, 128]
    assert all(sorted(h for D, h in P.BOUNDARY if D == dd) == [64, 65] for dd in (16, 64))
    for D, h0 in P.BOUNDARY:
        k = P.boundary_inputs(D, h0)
        _in_range(k)
        assert k["n"] == 1023 and k["layers"][0][0].shape == (h0, 2 * D) and k["layers"][1][0].shape == (D, h0)
        assert np.array_equal(np.unique(k["hlen"]), np.arange(k["T"] + 1))  # every length 0 .. T
        assert len(np.unique(k["uid"])) < k["n"] and not np.array_equal(k["uid"], np.arange(k["n"]))


def test_wave_loop_case_and_its_sample():
    k = P.loop_inputs(G, S.NOMINAL_CUS)
    _in_range(k)
    c = P.SAMPLE_CASE
    assert k["n"] == 3 * G * 32 * S.NOMINAL_CUS + 7 and (k["D"], k["h0"], k["T"]) == (32, 64, 30) == (c.D, c.widths[0], c.T)
    assert 0.25 < (k["hlen"] == 0).mean() < 0.35  # runs of empty histories meet in one pass
    sample = k["sample"]
    assert len(sample) == len(np.unique(sample)) == P.N_SAMPLE == c.n and sample[0] > 0 and sample[-1] < k["n"] - 1
    for ends in (0, k["T"]):
        hlen = P.loop_lens(k, ends)
        _in_range(k, hlen)
        assert hlen[0] == hlen[-1] == ends and np.array_equal(hlen[1:-1], k["hlen"][1:-1])
    # the rows held to the fp64 reference are SAMPLE_CASE's own, which
    # S.make_case conditioned, over its tables and layers
    k0 = S.make_case(c)
    assert k["ue"] is k0["ue"] and k["ie"] is k0["ie"] and k["layers"] is k0["layers"]
    assert all(np.array_equal(k[f][sample], k0[f]) for f in ("uid", "hist", "hlen"))
    # ... and meet what tests/test_tower_host.py requires of every case of that file
    assert H._e32(c) <= S.BAR_USER, H._e32(c)
    H.test_cases_see_a_one_slot_error(c)
    assert (k0["hlen"] >= 1).sum() > P.N_SAMPLE // 2


def test_dead_case():
    k = P.dead_inputs(G)
    _in_range(k)
    n, dead, nan_user = k["n"], k["dead"], k["nan_user"]
    assert n == 8 * G + 3 and np.array_equal(dead // G, np.arange(8)) and (dead % G == 1).all()  # one per whole pass
    assert nan_user not in dead and np.isnan(k["ue"][k["uid"][nan_user]]).any()
    finite = np.arange(n) != nan_user
    assert np.isfinite(k["ue"][k["uid"][finite]]).all()
    _, pres = oracle.tower_user_f64_parts(k["ue"], k["ie"], k["uid"][finite], k["hist"][finite], k["hlen"][finite],
                                          k["layers"])
    is_dead = np.isin(np.flatnonzero(finite), dead)
    assert pres[-1][is_dead].max() <= -1.0       # every last pre-activation, by a wide margin
    assert pres[-1][~is_dead].min() >= 0.5       # the others are alive in every output

"""Profile-feature checks that need no GPU: the vectorised restatement (the
checker of the GPU tests) equals reference-executed data bit for bit, as
shipped and with the word lookup repaired; the C entry points refuse bad
arguments before any launch; the ctypes table matches the header."""
import os
import re

import numpy as np
import pytest

from nrk import _lib

import profile_restated as rs


@pytest.fixture(scope="module")
def fx(golden):
    return golden("profile_small")


@pytest.fixture(scope="module")
def restated(fx):
    clicks, arts = rs.frames(fx)
    out = {}
    for prefix, repair in (("", False), ("fix_", True)):
        ucols, icols = rs.user_columns(clicks, arts, repair_word_lookup=repair), rs.item_columns(clicks, arts)
        out[prefix] = (ucols, icols) + rs.dicts(ucols, icols)
    return clicks, out


def test_fixture_cannot_hide_a_failure(fx):
    """The conditions the generator asserts, visible from the stored data."""
    clicks, arts = rs.frames(fx)
    n = clicks.groupby("user_id").size()
    assert (n == 1).any() and (n == 2).any() and n.max() >= 20
    assert clicks.duplicated(["user_id", "click_article_id"]).sum() >= 50
    top = clicks[clicks["click_timestamp"] == clicks.groupby("user_id")["click_timestamp"].transform("max")]
    assert (top.groupby("user_id")["click_article_id"].nunique() > 1).sum() >= 10
    sizes = clicks.groupby(["user_id", "click_deviceGroup"]).size()
    assert ((sizes == sizes.groupby("user_id").transform("max")).groupby("user_id").sum() > 1).sum() >= 20
    clicked, known = set(fx["click_item"].tolist()), set(fx["art_id"].tolist())
    assert len(known - clicked) >= 50 and len(clicked - known) == 2
    classes = fx["device_classes"].tolist()
    assert len(classes) >= 12 and classes.index("10.0") < classes.index("2.0")
    assert not fx["u_avg_word_count"].any() and (fx["fix_u_avg_word_count"] > 0).sum() > 250
    assert not clicks["user_id"].is_monotonic_increasing  # frame order is not user order
    assert 10 <= fx["labels"].sum() < len(fx["labels"]) and (fx["labels_online"] == -1).all()
    known_u = set(fx["click_user"].tolist())
    assert sum(u not in known_u for u in fx["pair_user"].tolist()) == 3
    assert sum(i not in known for i in fx["pair_item"].tolist()) >= 10


@pytest.mark.parametrize("prefix", ["", "fix_"])
def test_restated_dicts_equal_the_reference(fx, restated, prefix):
    _, _, user, items = restated[1][prefix]
    rs.check_dicts(fx, prefix, user, items)


@pytest.mark.parametrize("prefix", ["", "fix_"])
def test_restated_encoding_equals_the_reference(fx, restated, prefix):
    _, _, user, items = restated[1][prefix]
    ut, it, uvoc, ivoc = rs.encoded(user, items)
    assert np.array_equal(ut, fx[prefix + "user_table"]) and np.array_equal(it, fx[prefix + "item_table"])
    assert uvoc == fx[prefix + "user_vocab"].tolist() and ivoc == fx[prefix + "item_vocab"].tolist()
    assert ut.min() >= 1 and it.min() >= 1 and (ut.max(0) + 1).tolist() == uvoc and (it.max(0) + 1).tolist() == ivoc


def test_restated_labels_equal_the_reference(fx, restated):
    clicks = restated[0]
    got = rs.labels(clicks, fx["pair_user"], fx["pair_item"])
    assert np.array_equal(got, fx["labels"]) and np.array_equal(got, fx["fix_labels"])
    assert np.array_equal(rs.labels(clicks, fx["pair_user"], fx["pair_item"], offline=False), fx["labels_online"])


def test_argument_errors():
    L = _lib.lib()
    err = lambda: L.nrk_last_error()  # noqa: E731
    E, U = _lib.NRK_EINVAL, _lib.NRK_EUNSUPPORTED

    def user(n_users=3, n_clicks=10, n_codes=4, n_items=5):
        return L.nrk_profile_user(None, n_users, None, None, None, n_clicks, n_codes, None, None, n_items,
                                  None, None, None, None, None, None, None)

    assert user() == E and b"nrk_profile_user: null pointer" in err()
    for kw in ("n_users", "n_clicks", "n_codes", "n_items"):
        assert user(**{kw: -1}) == E and b"nrk_profile_user: negative size" in err(), kw
    assert user(n_clicks=2**31) == E and b"2^31" in err()
    assert user(n_items=2**31) == E and b"2^31" in err()
    assert user(n_codes=64) == E and b"null pointer" in err()
    assert user(n_codes=65) == U and b"nrk_profile_user: more than 64 device-group codes" in err()
    with pytest.raises(NotImplementedError):
        _lib.check(user(n_codes=65), "nrk_profile_user")

    count = lambda n_clicks=10, n_items=5: L.nrk_profile_item_count(None, n_clicks, n_items, None, None)  # noqa: E731
    assert count() == E and b"nrk_profile_item_count: null pointer" in err()
    assert count(n_clicks=-1) == E and b"negative size" in err()
    assert count(n_items=-1) == E and b"negative size" in err()
    assert count(n_items=2**31) == E and b"2^31" in err()
    assert count(n_clicks=0, n_items=0) == _lib.NRK_OK

    scale = lambda n=10, skip=0: L.nrk_profile_scale(None, n, None, skip, None, None)  # noqa: E731
    assert scale() == E and b"nrk_profile_scale: null pointer" in err()
    assert scale(n=-1) == E and b"negative size" in err()
    assert scale(skip=2) == E and b"skip_zero must be 0 or 1" in err()
    assert scale(n=0) == _lib.NRK_OK

    labels = lambda n=10, n_users=3, off=1: L.nrk_profile_labels(None, None, n, None, n_users, off, None, None)  # noqa: E731
    assert labels() == E and b"nrk_profile_labels: null pointer" in err()
    assert labels(off=0) == E and b"null pointer" in err()  # the output
    assert labels(n=-1) == E and b"negative size" in err()
    assert labels(n_users=-1) == E and b"negative size" in err()
    assert labels(off=2) == E and b"offline must be 0 or 1" in err()
    assert labels(n=0) == _lib.NRK_OK
    with pytest.raises(ValueError):
        _lib.check(labels(), "nrk_profile_labels")
    assert L.nrk_abi_version() == 3


C_TYPES = {"int": _lib.INT, "int64_t": _lib.I64, "double": _lib.F64, "nrk_stream_t": _lib.P}


def test_signatures_match_the_header():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nrk.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = re.findall(r"\bint (nrk_profile_\w+)\(([^)]*)\);", hdr)
    assert sorted(n for n, _ in names) == ["nrk_profile_item_count", "nrk_profile_labels", "nrk_profile_scale",
                                           "nrk_profile_user"]
    for name, args in names:
        want = []
        for a in args.split(","):
            a = a.strip()
            want.append(_lib.P if "*" in a else C_TYPES[a.rsplit(" ", 1)[0].replace("const ", "")])
        res, got = _lib.SIGNATURES[name]
        assert res is _lib.INT and got == want, name

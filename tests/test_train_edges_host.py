"""The inputs of the trainer edge tests (test_gpu_tower_train_edges.py,
test_gpu_din_train_edges.py), built and checked without a GPU.

The GPU tests hold the kernels to 8 e_ref, e_ref = max |fp32 restatement -
fp64 restatement|.  That bar means something only if the inputs keep three
conditions, asserted here on the CPU for every new case:

1. tower: no row of either table receives more than 256 contributions in a
   batch (np.bincount over s_user, and over s_target with the gathered history
   items): the fp32 bar was sized for up to 256 terms in another order;
2. every compared tensor has e_ref > 0: a zero yardstick would turn the bar
   into bit-equality with fp64.  For the losses -- four scalars -- it must
   also be at least half an fp32 ulp of the loss: a value correctly rounded
   to fp32 is already off by up to half an ulp, so a smaller e_ref says only
   that all four fp32 sums happened to round correctly and measures no
   summation error (seen: 8.4e-9 on losses of 0.69, ulp 6.0e-8).  A generator
   whose losses miss that draws its case again from the next seed; the
   decision reads the two restatements alone;
3. DIN: no Dice column has batch std 0 (out of contract, din_train.hip).

The generators live here because both GPU files and this one share them; each
is deterministic in its arguments.  Every figure is printed before it is
asserted.
"""
import functools
import types

import numpy as np
import pytest
import torch

import din_train_restated as RD
import tower_train_restated as RT
from test_gpu_din_train import vocabs_for
from test_gpu_tower_train import make_batch, make_log

TR_CT, TR_KEYS, TR_MAXB, DT_PIECE = 4096, 8192, 8192, 512  # csrc/tower_train.hip, csrc/din_train.hip
MAX_TERMS = 256


def chunk_size(T):
    """tr_layout: samples one workgroup sorts."""
    return min(256, TR_KEYS // (T + 1))


def loss_yardstick(l32, l64):
    """(e_ref of the losses, the least it may be: half an fp32 ulp of the largest loss)."""
    return RT.err(l32, l64), 0.5 * float(np.spacing(np.float32(np.max(np.abs(l64)))))


def settle(build, losses):
    """build(attempt) for attempt = 0, 1, ... until the case's losses give a
    yardstick of at least half an ulp (condition 2); ``losses(case, dtype)``
    runs the restatement's forward."""
    for attempt in range(16):
        case = build(attempt)
        e, least = loss_yardstick(losses(case, torch.float32), losses(case, torch.float64))
        if e >= least:
            return case
    raise AssertionError("no case with a loss yardstick of half an ulp in 16 draws")


def tower_losses(case, dtype):
    return [RT.loss_only(case.state, case.off, case.items, b, case.T, dtype, m, case.p)
            for b, m in zip(case.batches, case.masks)]


def din_losses(case, dtype):
    return [RD.loss_only(case[0], case[1], b, dtype) for b in case[2]]


# ------------------------------------------------------------------ tower --
def _case(state, off, items, batches, T, **kw):
    return types.SimpleNamespace(state=state, off=off, items=items, batches=batches, T=T, kw=kw,
                                 U=len(off) - 1, I=state["item_embedding.weight"].shape[0],
                                 masks=[None] * len(batches), p=kw.get("p", 0.0))


def boundary_rows(n):
    """Rows at the edges of the TR_CT compaction tiles of a table of n rows,
    and one row in every tenth tile."""
    rows = {0, TR_CT - 1, TR_CT, TR_CT + 1, 2 * TR_CT - 1, 2 * TR_CT, n - 1}
    rows |= {t * TR_CT + 17 for t in range(0, (n + TR_CT - 1) // TR_CT, 10)}
    return np.array(sorted(r for r in rows if 0 <= r < n), np.int64)


COMPACTION = [(4096, 4097), (8192, 300), (300, 12289), (270000, 4097), (4097, 270000)]
COMPACTION_B, COMPACTION_T, RECUR = 700, 64, 20


@functools.lru_cache(maxsize=2)
def compaction_case(U, I):
    """B = 700 at T = 64 (six chunks of 126).  Twenty users and twenty targets
    recur in every chunk; every boundary row of both tables is hit as a user,
    as a target and as a history item.  Recurring and boundary users have log
    rows of 66 .. 90 clicks, so their histories fill all 64 lanes.

    Each recurring user has six clones: users with the same embedding row and
    the same log row that no batch samples.  ``probe`` is the first batch with
    the recurring user's sample in chunk c handed to its c-th clone, so a call
    on it returns every term of the recurring user's gradient separately
    (a sample's gradient depends on its user's values, not on its id)."""
    B, T, CS = COMPACTION_B, COMPACTION_T, chunk_size(COMPACTION_T)
    n_chunks = (B + CS - 1) // CS
    return settle(lambda attempt: _compaction(U, I, B, T, CS, n_chunks, np.random.default_rng([U, I, attempt])),
                  tower_losses)


def _compaction(U, I, B, T, CS, n_chunks, rng):
    D, hidden = (16, [16]) if max(U, I) > 100000 else (32, [64, 32])
    su, si = boundary_rows(U), boundary_rows(I)
    picked = rng.choice(np.setdiff1d(np.arange(U), su), RECUR * (1 + n_chunks), replace=False)
    ru, clones = picked[:RECUR], picked[RECUR:].reshape(RECUR, n_chunks)
    rt = rng.choice(I, RECUR, replace=False)
    heavy = np.concatenate([su, ru])
    lens = rng.integers(2, 91, U) if U <= 10000 else rng.integers(2, 8, U)
    lens[heavy] = rng.integers(66, 91, len(heavy))
    lens[clones] = lens[ru][:, None]
    off, items = RT.log_with_lengths(rng, lens, I)
    assert len(si) <= len(heavy)
    items[off[heavy[:len(si)]]] = si  # the first click of a heavy user's row: every sample of that user gathers it
    state = RT.random_state(rng, U, I, D, hidden, bias_scale=0.05)
    for r, cs in zip(ru, clones):
        for c in cs:
            items[off[c]:off[c + 1]] = items[off[r]:off[r + 1]]
            state["user_embedding.weight"][c] = state["user_embedding.weight"][r]
    pool = np.setdiff1d(np.arange(U), picked)  # the other samples' users: a recurring user has exactly six samples
    batches = []
    for _ in range(4):
        u = pool[rng.integers(0, len(pool), B)]
        pos = 1 + rng.integers(0, 1 << 30, B) % lens[u]
        tgt, lab = rng.integers(0, I, B), rng.integers(0, 2, B).astype(np.float32)
        for c in range(n_chunks):
            u[c * CS:c * CS + RECUR] = ru
            pos[c * CS:c * CS + RECUR] = 1 + rng.integers(0, 1 << 30, RECUR) % lens[ru]
            tgt[c * CS + RECUR:c * CS + 2 * RECUR] = rt
        u[2 * RECUR:2 * RECUR + len(su)] = su  # chunk 0
        pos[2 * RECUR:2 * RECUR + len(su)] = lens[su]
        tgt[CS + 2 * RECUR:CS + 2 * RECUR + len(si)] = si  # chunk 1
        batches.append((u.astype(np.int64), pos.astype(np.int64), tgt.astype(np.int64), lab))
    case = _case(state, off, items, batches, T)
    case.su, case.si, case.ru, case.rt, case.clones = su, si, ru, rt, clones
    pu = batches[0][0].copy()
    for c in range(n_chunks):
        pu[c * CS:c * CS + RECUR] = clones[:, c]
    case.probe = (pu,) + batches[0][1:]
    return case


@functools.lru_cache(maxsize=1)
def bench_shape_case():
    """tools/tower_train_bench.py's shape: 62 user tiles and 89 item tiles,
    B = 4096 uniform samples at T = 30 (17 chunks)."""
    U, I, B = 250000, 364047, 4096

    def build(attempt):
        rng = np.random.default_rng([250000, attempt])
        off, items = make_log(rng, U, I)
        state = RT.random_state(rng, U, I, 32, [64, 32], bias_scale=0.05)
        return _case(state, off, items, [make_batch(rng, off, I, B) for _ in range(4)], 30)

    return settle(build, tower_losses)


CHUNK_EDGES = [(30, 257), (30, 512), (30, 513), (32, 249), (32, 497), (1, 300), (63, 129), (64, 127), (30, TR_MAXB)]


@functools.lru_cache(maxsize=2)
def chunk_case(T, B):
    """Rows of 2 .. 90 clicks; the four longest rows are sampled at their full
    length (s_pos far above T; at T = 64 all 64 lanes gather) in the first
    sample, the last sample of the first chunk, the middle and the last sample
    of the batch."""
    return settle(lambda attempt: _chunk(T, B, np.random.default_rng([T, B, attempt])), tower_losses)


def _chunk(T, B, rng):
    U, I = (9000, 5000) if B == TR_MAXB else (600, 5000)
    off, items = make_log(rng, U, I, 2, 90)
    lens = off[1:] - off[:-1]
    state = RT.random_state(rng, U, I, 32, [64, 32], bias_scale=0.05)
    longest = np.argsort(lens, kind="stable")[-4:]
    where = [0, min(chunk_size(T), B) - 1, B // 2, B - 1]
    batches = []
    for _ in range(4):
        u, pos, tgt, lab = make_batch(rng, off, I, B)
        u[where], pos[where] = longest, lens[longest]
        batches.append((u, pos, tgt, lab))
    return _case(state, off, items, batches, T)


WIDTHS = {"256-32": (32, [256, 32]), "128-256-32": (32, [128, 256, 32]), "65-32": (32, [65, 32]), "1-32": (32, [1, 32]),
          "eight": (32, [40, 36, 33, 64, 48, 17, 96, 32]), "256-16": (16, [256, 16]), "60-64": (64, [60, 64]),
          "64-64": (64, [64, 64]), "dropout": (32, [256, 128, 32])}
DROPOUT = dict(p=0.5, seed=77, step=12)


@functools.lru_cache(maxsize=2)
def width_case(name):
    """B = 37, 50 users, 80 items, T = 30.  "dropout": p = 0.5, the keep masks
    restated on the CPU (tower_train_restated.dropout_mask)."""
    D, hidden = WIDTHS[name]
    return settle(lambda attempt: _width(name, D, hidden, np.random.default_rng([D, len(hidden), hidden[0], attempt])),
                  tower_losses)


def _width(name, D, hidden, rng):
    B, U, I, T = 37, 50, 80, 30
    off, items = make_log(rng, U, I)
    state = RT.random_state(rng, U, I, D, hidden, bias_scale=0.05)
    case = _case(state, off, items, [make_batch(rng, off, I, B) for _ in range(4)], T,
                 **(DROPOUT if name == "dropout" else {}))
    if name == "dropout":  # the masks depend on (seed, step, layer, sample, unit), not on the batch
        case.masks = [[RT.dropout_mask(DROPOUT["seed"], DROPOUT["step"], l, B, w, DROPOUT["p"])
                       for l, w in enumerate(hidden)]] * 4
    return case


def staged(D, hidden):
    """nrk_tt_train_grad: (weights ride in LDS?, dynamic LDS bytes)."""
    asz, floats, fan_in = 2 * D + sum(hidden), 0, 2 * D
    for w in hidden:
        floats += w * (fan_in + 2)
        fan_in = w
    wave = 4 * (asz + 2 * 256)
    fits = (wave + floats) * 4 <= 60 * 1024
    return fits, 4 * (wave + (floats if fits else 0))


def tower_refs(case):
    """Per batch (loss, gradients) of the fp32 and of the fp64 restatement.
    Only the first batch's gradients are compared, so the others run the
    forward alone -- unless a parameter has one element: its gradient is
    compared over all batches, as the losses are."""
    scalar = any(np.size(v) == 1 for v in case.state.values())
    out = []
    for dt in (torch.float32, torch.float64):
        rs = []
        for n, (b, m) in enumerate(zip(case.batches, case.masks)):
            if n == 0 or scalar:
                rs.append(RT.grads(case.state, case.off, case.items, b, case.T, dt, m, case.p))
            else:
                rs.append((RT.loss_only(case.state, case.off, case.items, b, case.T, dt, m, case.p), None))
        out.append(rs)
    return out


def tower_touched(case, batch):
    """(user rows, item rows) a batch's gradient must list: np.unique of the touched rows."""
    return np.unique(batch[0]), np.unique(np.concatenate([batch[2], RT.gathered_items(case.off, case.items, batch[0],
                                                                                      batch[1], case.T)]))


def max_contributions(case, batch):
    users = np.bincount(batch[0], minlength=case.U)
    item_terms = np.concatenate([batch[2], RT.gathered_items(case.off, case.items, batch[0], batch[1], case.T)])
    return int(users.max()), int(np.bincount(item_terms, minlength=case.I).max())


def check_tower_inputs(what, case):
    """Conditions 1 and 2 for one tower case."""
    for n, b in enumerate(case.batches):
        mu, mi = max_contributions(case, b)
        print(f"{what} batch {n}: most contributions to a user row {mu}, to an item row {mi}")
        assert mu <= MAX_TERMS and mi <= MAX_TERMS
        lens = case.off[b[0] + 1] - case.off[b[0]]
        assert (b[1] >= 1).all() and (np.minimum(b[1], case.T) <= lens).all()
    r32, r64 = tower_refs(case)
    zero = []
    for k, g64 in r64[0][1].items():
        if g64.size == 1:
            e = RT.err([r[1][k] for r in r32], [r[1][k] for r in r64])
        else:
            e = RT.err(r32[0][1][k], g64)
        print(f"{what} e_ref {k}: {e:.3e}")
        zero += [k] * (not e > 0)
    e, least = loss_yardstick([r[0] for r in r32], [r[0] for r in r64])
    print(f"{what} e_ref losses: {e:.3e} (half an ulp: {least:.3e})")
    assert e >= least > 0 and not zero, zero


@pytest.mark.parametrize("U,I", COMPACTION)
def test_compaction_inputs(U, I):
    """TR_CT: the forced rows are where the case says they are."""
    case = compaction_case(U, I)
    CS = chunk_size(case.T)
    assert CS == 126 and -(-COMPACTION_B // CS) == 6
    for b in case.batches:
        users, rows = tower_touched(case, b)
        hist = np.unique(RT.gathered_items(case.off, case.items, b[0], b[1], case.T))
        assert np.isin(case.su, users).all() and np.isin(case.si, b[2]).all() and np.isin(case.si, hist).all()
        for c in range(6):
            chunk = slice(c * CS, (c + 1) * CS)
            assert np.isin(case.ru, b[0][chunk]).all() and np.isin(case.rt, b[2][chunk]).all()
        assert (b[1] >= 64).sum() >= len(case.su)
        assert (np.bincount(b[0], minlength=U)[case.ru] == 6).all() and not np.isin(case.clones, b[0]).any()
        tiles_u, tiles_i = np.unique(users // TR_CT), np.unique(rows // TR_CT)
        print(f"U={U} I={I}: {len(users)} user rows in {len(tiles_u)} of {-(-U // TR_CT)} tiles, "
              f"{len(rows)} item rows in {len(tiles_i)} of {-(-I // TR_CT)} tiles")
        assert tiles_u[-1] == (U - 1) // TR_CT and tiles_i[-1] == (I - 1) // TR_CT
    b, pr = case.batches[0], case.probe
    moved = b[0] != pr[0]
    assert moved.sum() == 6 * RECUR and np.array_equal(np.sort(pr[0][moved]), np.sort(case.clones.reshape(-1)))
    for r, cs in zip(case.ru, case.clones):
        for c in cs:
            assert np.array_equal(case.items[case.off[c]:case.off[c + 1]], case.items[case.off[r]:case.off[r + 1]])
            assert np.array_equal(case.state["user_embedding.weight"][c], case.state["user_embedding.weight"][r])
    check_tower_inputs(f"compaction U={U} I={I}", case)


def test_bench_shape_inputs():
    """The fp64 dense pass over 250,000 + 364,047 rows of 32 takes a few
    seconds on the CPU and is kept."""
    case = bench_shape_case()
    assert -(-case.U // TR_CT) == 62 and -(-case.I // TR_CT) == 89
    check_tower_inputs("bench shape", case)


@pytest.mark.parametrize("T,B", CHUNK_EDGES)
def test_chunk_edge_inputs(T, B):
    case = chunk_case(T, B)
    CS = chunk_size(T)
    print(f"T={T} B={B}: CS {CS}, {-(-B // CS)} chunks, last chunk {B - (B - 1) // CS * CS} samples")
    assert CS == {30: 256, 32: 248, 1: 256, 63: 128, 64: 126}[T] and B > CS
    assert all((b[1] - T).max() >= 20 and (b[1] >= 64).any() for b in case.batches)
    check_tower_inputs(f"chunks T={T} B={B}", case)


@pytest.mark.parametrize("name", list(WIDTHS))
def test_width_inputs(name):
    case = width_case(name)
    D, hidden = WIDTHS[name]
    fits, lds = staged(D, hidden)
    print(f"{name}: D {D} hidden {hidden} staged {fits} LDS {lds} B")
    assert fits == (name in ("65-32", "1-32", "60-64")) and lds <= 64 * 1024
    if name == "60-64":
        assert lds == 59296
    if name == "64-64":
        assert (4 * (2 * 64 + 128 + 512) + 64 * 130 + 64 * 66) * 4 == 62464 and lds == 4 * 4 * (2 * 64 + 128 + 512)
    if name == "dropout":
        keep = np.mean([m.mean() for m in case.masks[0]])
        print(f"dropout keep rate {keep:.4f}")
        assert all(set(np.unique(m)) == {0.0, 1.0} for m in case.masks[0]) and abs(keep - 0.5) < 0.02
    check_tower_inputs(f"widths {name}", case)


SAMPLE_LENGTHS = [0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 60]
SAMPLE_USERS = [1, 2, 1023, 1024, 1025, 2049]


def sample_log(U, short=False):
    """Rows whose lengths run through SAMPLE_LENGTHS (longest first, so U = 1
    has positives), in shuffled order; ``short``: at most 2 clicks a row, so
    no row has a positive."""
    rng = np.random.default_rng([U, short])
    lens = rng.permutation(np.resize([0, 1, 2] if short else SAMPLE_LENGTHS[::-1], U))
    return RT.log_with_lengths(rng, lens, 1000)


@pytest.mark.parametrize("U", SAMPLE_USERS)
def test_sample_logs(U):
    off, _ = sample_log(U)
    lens = off[1:] - off[:-1]
    pos = RT.positives(off)
    per_user = np.bincount(pos[:, 0], minlength=U) if len(pos) else np.zeros(U, np.int64)
    expect = {0: 0, 1: 0, 2: 0, 3: 1, 4: 2, 5: 3, 6: 4, 9: 7, 10: 7, 11: 8, 60: 47}
    assert all(per_user[u] == expect[int(n)] for u, n in enumerate(lens)) and len(pos) > 0
    assert len(RT.positives(sample_log(U, short=True)[0])) == 0


# -------------------------------------------------------------------- DIN --
def din_case(seed, vocabs, hidden, B, T, full=False, distinct=False, edit=None):
    """(state, feats, four batches); ``edit(batch, rng)`` forces a case's special indices."""
    def build(attempt):
        rng = np.random.default_rng(list(np.atleast_1d(seed)) + [attempt])
        state, feats = RD.random_state(rng, vocabs, hidden)
        batches = [RD.random_batch(rng, vocabs, B, T, full=full, distinct=distinct) for _ in range(4)]
        for b in batches:
            if edit:
                edit(b, rng)
        return state, feats, batches

    return settle(build, din_losses)


NI8_SHAPES = [(2, 1), (37, 7), (64, 50), (16, 128), (300, 20)]


def ni8_case(B, T):
    """dt_run<8>; B = 2 with distinct candidates and full histories (no Dice column of std 0)."""
    return din_case([8, B, T], vocabs_for(8), (40, 24), B, T, full=B == 2, distinct=B == 2)


def t_edge_case(n_item, T):
    return din_case([n_item, T], vocabs_for(n_item), (40, 24), 24, T)


def no_ctx_case():
    return din_case(70, vocabs_for(2, n_user=1, n_ctx=0), (40, 24), 37, 7)


def max_feats_case():
    """DT_MAXF: 64 user and 64 context features, each of vocabulary 3."""
    vocabs = ({f"u{i}": 3 for i in range(64)}, vocabs_for(2)[1], {f"c{i}": 3 for i in range(64)})
    return din_case(64, vocabs, (40, 24), 16, 3)


MLP_SHAPES = [(24, 200), (1, 1), (1024, 1), (17, 1024), (64, 64), (65, 63)]


def mlp_case(hidden):
    return din_case([hidden[0], hidden[1]], vocabs_for(2), hidden, 37, 7)


KSPLIT_B = [511, 512, 513, 8192]


def ksplit_case(B):
    return din_case([B, 2], vocabs_for(1), (40, 24), B, 2)


PIECE_COUNTS = [512, 513, 1024, 1025, 511]  # occurrences of values 0 .. 4 of the first user feature
PIECE_STARTS = [0, 512, 1025, 2049, 3074]


def piece_case():
    """DT_PIECE: the first user feature's rows sort first, so its values 0 ..
    4 are the sorted segments [0, 512), [512, 1025), [1025, 2049), [2049, 3074)
    and [3074, 3585): an exact-fit direct segment (en - st == DT_PIECE), a long
    segment that starts on a tile boundary with a one-term second piece, a
    segment of two full pieces whose last term is the first of a tile, a
    three-piece segment with a one-term tail, and a direct segment one short
    of a piece."""
    B = 4000
    vocabs = ({"u0": 12, "u1": 23}, {"i0": 24}, {f"c{i}": 5 + i for i in range(3)})
    fixed = np.repeat(np.arange(5), PIECE_COUNTS)

    def edit(b, rng):
        b["user"][:, 0] = rng.permutation(np.concatenate([fixed, rng.integers(5, 12, B - len(fixed))]))

    return din_case(512, vocabs, (40, 24), B, 1, full=True, edit=edit)


TABLE_ROWS = [1023, 1024, 1025]


def table_rows_case(R):
    """dt_sort_bits: 2^10 - 1, 2^10 and 2^10 + 1 table rows, the last one touched."""
    vocabs = ({"u0": 400, "u1": 300}, {"i0": 200}, {"c0": R - 900})
    def edit(b, rng):
        b["ctx"][0, 0] = R - 900 - 1

    return din_case(R, vocabs, (40, 24), 64, 5, edit=edit)


def check_din_inputs(what, state, feats, batches):
    """Conditions 2 and 3 for one DIN case."""
    sd = min(RD.min_dice_std(state, feats, b) for b in batches)
    print(f"{what}: smallest Dice column std {sd:.3e}")
    assert sd > 0
    r32 = [RD.grads(state, feats, b, torch.float32) for b in batches]
    r64 = [RD.grads(state, feats, b, torch.float64) for b in batches]
    zero = []
    for k, g64 in r64[0][1].items():
        e = RD.err([r[1][k] for r in r32], [r[1][k] for r in r64]) if g64.size == 1 else RD.err(r32[0][1][k], g64)
        print(f"{what} e_ref {k}: {e:.3e}")
        zero += [k] * (not e > 0)
    e, least = loss_yardstick([r[0] for r in r32], [r[0] for r in r64])
    print(f"{what} e_ref losses: {e:.3e} (half an ulp: {least:.3e})")
    assert e >= least > 0 and not zero, zero


@pytest.mark.parametrize("B,T", NI8_SHAPES + [(100, 50)])
def test_ni8_inputs(B, T):
    check_din_inputs(f"n_item=8 B={B} T={T}", *ni8_case(B, T))


@pytest.mark.parametrize("T", [64, 65, 128])
@pytest.mark.parametrize("n_item", [1, 2, 4])
def test_t_edge_inputs(n_item, T):
    check_din_inputs(f"n_item={n_item} T={T}", *t_edge_case(n_item, T))


def test_feature_count_inputs():
    check_din_inputs("n_ctx=0", *no_ctx_case())
    state, feats, batches = max_feats_case()
    assert len(feats[0]) == 64 and len(feats[2]) == 64
    check_din_inputs("64 user + 64 ctx features", state, feats, batches)


@pytest.mark.parametrize("hidden", MLP_SHAPES)
def test_mlp_shape_inputs(hidden):
    check_din_inputs(f"hidden={hidden}", *mlp_case(hidden))


@pytest.mark.parametrize("B", KSPLIT_B)
def test_ksplit_inputs(B):
    print(f"B={B}: ksplit {max(1, min(16, B // 256))}")
    check_din_inputs(f"ksplit B={B}", *ksplit_case(B))


def test_piece_inputs():
    state, feats, batches = piece_case()
    for b in batches:
        counts = np.bincount(b["user"][:, 0], minlength=12)
        assert list(counts[:5]) == PIECE_COUNTS and counts[5:].min() > 0
        assert list(np.concatenate([[0], np.cumsum(counts[:4])])) == PIECE_STARTS
    assert PIECE_COUNTS[0] == DT_PIECE and PIECE_STARTS[1] % DT_PIECE == 0
    check_din_inputs("pieces", state, feats, batches)


@pytest.mark.parametrize("R", TABLE_ROWS)
def test_table_rows_inputs(R):
    state, feats, batches = table_rows_case(R)
    assert sum(state[k].shape[0] for k in RD.state_keys(feats) if "embedding_dict" in k) == R
    check_din_inputs(f"R={R}", state, feats, batches)

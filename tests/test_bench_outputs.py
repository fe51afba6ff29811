"""bench.py --dump-outputs / --full: a plain run measures the headline alone
and can write what its last timed step computed; the other legs run with
--full.  The sampling helpers are checked on the CPU, one small run of the
benchmark itself (in this process) on the GPU."""
import json
import os

import numpy as np
import pytest
import torch

import bench


def test_dump_rows_fixed_sample_within_budget():
    assert bench.dump_rows(1000, 376) is None  # fits: every row
    assert bench.dump_rows(10, 100, budget=1000) is None  # exactly the budget
    a = bench.dump_rows(250_000, 376)
    assert len(a) * 376 <= bench.DUMP_BUDGET_BYTES < 64_000_000
    assert len(a) == bench.DUMP_BUDGET_BYTES // 376
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 250_000  # sorted, no repeats, in range
    assert np.array_equal(a, bench.dump_rows(250_000, 376))  # the same rows every run


def test_dump_outputs_writes_float32_rows(tmp_path):
    s = torch.arange(12, dtype=torch.float32).view(6, 2) / 7
    r = torch.arange(18, dtype=torch.int32).view(6, 3)
    assert bench.dump_outputs(str(tmp_path / "d"), {"s": s, "r": r}) is None
    got_s, got_r = np.load(tmp_path / "d" / "s.npy"), np.load(tmp_path / "d" / "r.npy")
    assert got_s.dtype == np.float32 and got_r.dtype == np.float32
    assert np.array_equal(got_s, s.numpy()) and np.array_equal(got_r, r.numpy())
    # over the budget: the same sampled rows of every array, in order
    rows = bench.dump_outputs(str(tmp_path / "e"), {"s": s, "r": r}, budget=60)
    assert len(rows) == 3 and np.array_equal(rows, bench.dump_rows(6, 20, budget=60))
    assert np.array_equal(np.load(tmp_path / "e" / "s.npy"), s.numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "e" / "r.npy"), r.numpy()[rows])
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "f"), {"s": s, "r": r[:5]})  # one row per user in every array


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(tmp_path, capsys):
    """A plain run at a small size: the result line has the headline fields
    and none of the --full legs, and the dumped arrays are the oracle's
    (rows and scores exact, the tower to 1e-5 as in smoke())."""
    from oracle import oracle

    U, I, D, k = 1100, 5003, 32, 30
    d = str(tmp_path / "out")
    bench.main(["--gpus", "1", "--steps", "2", "--warmup", "1", "--users", str(U), "--items", str(I),
                "--dump-outputs", d])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["unit"] == "recalled pairs/s"
    assert line["value"] == pytest.approx(U * k / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert all(line[f] is None for f in ("cpu_baseline", "din", "itemcf", "plugins", "config4"))
    assert sorted(os.listdir(d)) == ["topk_rows.npy", "topk_scores.npy", "user_vec.npy"]
    u, s, r = (np.load(os.path.join(d, n + ".npy")) for n in ("user_vec", "topk_scores", "topk_rows"))
    assert u.dtype == s.dtype == r.dtype == np.float32
    assert u.shape == (U, D) and s.shape == (U, k + 1) and r.shape == (U, k + 1)
    wl = {n: (t.cpu().numpy() if torch.is_tensor(t) else t)
          for n, t in bench.recall_workload(23, U, I, D, "cpu").items()}
    ur = oracle.tower_user(wl["user_table"], wl["item_table"], wl["uid"], wl["hist"], wl["hist_len"],
                           wl["w0"], wl["b0"], wl["w1"], wl["b1"])
    assert np.allclose(u, ur, atol=1e-5)
    # the catalog the benchmark searched: the item tower's own output
    from nrk import ops

    it = ops.tt_item_fwd(torch.from_numpy(wl["item_table"]).cuda(), torch.arange(I, dtype=torch.int32, device="cuda"))
    assert np.allclose(it.cpu().numpy(), oracle.tower_item(wl["item_table"], np.arange(I)), atol=1e-6)
    so, ro = oracle.ip_topk(u, it.cpu().numpy(), k + 1)
    assert np.array_equal(r, ro) and np.array_equal(s, so)

"""bench.py --dump-outputs on the host: one float64 file per output, and beyond the size limit the same fixed, seeded sample of
patterns from every per-pattern array."""
import numpy as np

import bench


def _sites(P, C=4):
    r = np.random.default_rng(1)
    return {"c_lnL_sorted": r.normal(size=P), "cur_site_lk": r.random(P), "unscaled_site_lk_cat": r.random((P, C)),
            "fact_sum_scale": r.integers(0, 3, P).astype(np.float64)}


def test_dump_outputs_whole(tmp_path):
    s = _sites(1000)
    bench.dump_outputs(str(tmp_path), -123.5, s)
    assert sorted(f.name for f in tmp_path.iterdir()) == sorted(["lnL.npy"] + [k + ".npy" for k in s])
    lnl = np.load(tmp_path / "lnL.npy")
    assert lnl.dtype == np.float64 and lnl.tolist() == [-123.5]
    for k, v in s.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v), k


def test_dump_outputs_sample_beyond_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1 << 20)
    s = _sites(50000)  # 56 bytes per pattern: 2.8 MB in all
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), -1.0, s)
    a = tmp_path / "a"
    assert sum(f.stat().st_size for f in a.iterdir()) <= 1 << 20
    idx = np.load(a / "pattern_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "pattern_index.npy"))  # a fixed sample
    idx = idx.astype(np.int64)
    assert len(idx) > 15000 and np.all(np.diff(idx) > 0) and idx[-1] < 50000
    for k, v in s.items():
        assert np.array_equal(np.load(a / (k + ".npy")), v[idx]), k
    assert np.load(a / "lnL.npy").tolist() == [-1.0]

"""bench.py --dump-outputs (bench.dump_outputs): float64 .npy files, whole arrays while they fit the size limit, else a
fixed seeded sample of the oversized ones -- the same elements in every run.  CPU only: no GPU call."""
import os
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_arrays_that_fit_are_written_whole(tmp_path):
    cons = np.arange(2 * 5 * 5, dtype=np.float64).reshape(2, 5, 5) / 7
    labels = np.arange(12, dtype=np.int32).reshape(3, 4)
    bench.dump_outputs(str(tmp_path / "o"), {"consensus": cons, "labels": labels, "rho": [0.5, 1.0], "absent": None})
    got = _load(tmp_path / "o")
    assert sorted(got) == ["consensus", "labels", "rho"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["consensus"], cons) and np.array_equal(got["labels"], labels)
    assert np.array_equal(got["rho"], [0.5, 1.0])


def test_oversized_arrays_are_sampled_the_same_way_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 200)
    big = np.random.default_rng(1).random((30, 30))      # 900 elements, share = 100
    small = np.arange(10.0)
    bench.dump_outputs(str(tmp_path / "a"), {"big": big, "small": small})
    bench.dump_outputs(str(tmp_path / "b"), {"big": big, "small": small})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 8 * 200
    assert a["big"].shape == (100,) and np.array_equal(a["big"], b["big"])
    assert np.isin(a["big"], big).all() and len(np.unique(a["big"])) == 100
    assert np.array_equal(a["small"], small)
    changed = big.copy()
    changed += 1.0                                        # another build's output differs everywhere: the sample shows it
    bench.dump_outputs(str(tmp_path / "c"), {"big": changed, "small": small})
    assert np.array_equal(_load(tmp_path / "c")["big"], a["big"] + 1.0)

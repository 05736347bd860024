"""bench.py --dump-outputs: what dump_outputs writes and how an array beyond its cap is sampled (host only)."""
import os

import numpy as np
import pytest
import torch

import bench


def test_dump_outputs_writes_whole_arrays_as_float32(tmp_path):
    grad = torch.randn(2, 3, 4, generator=torch.Generator().manual_seed(1))
    w = bench.dump_outputs(str(tmp_path), {"loss": torch.tensor(3.5), "nll": torch.arange(6), "grad": grad})
    assert w == {"loss": [], "nll": [6], "grad": [2, 3, 4]}
    assert sorted(os.listdir(tmp_path)) == ["grad.npy", "loss.npy", "nll.npy"]
    g, nll, loss = (np.load(tmp_path / (n + ".npy")) for n in ("grad", "nll", "loss"))
    assert g.dtype == nll.dtype == loss.dtype == np.float32
    assert np.array_equal(g, grad.numpy()) and np.array_equal(nll, np.arange(6)) and loss.shape == () and loss == 3.5


def test_dump_outputs_samples_an_array_beyond_the_cap_the_same_way_every_run(tmp_path):
    big = torch.arange(10000, dtype=torch.float64)
    cap = 10 * 4 + 600 * 8
    for run in ("a", "b"):
        w = bench.dump_outputs(str(tmp_path / run), {"small": torch.ones(10), "big": big}, cap_bytes=cap, sample=500)
        assert w["small"] == [10] and 0 < w["big_sample"][0] <= 500
        assert sorted(os.listdir(tmp_path / run)) == ["big_sample.npy", "small.npy"]
    a, b = (np.load(tmp_path / run / "big_sample.npy") for run in ("a", "b"))
    assert a.dtype == np.float64 and np.array_equal(a, b)
    # big[i] == i: the sample holds the positions it was taken at
    assert np.array_equal(a, np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, 10000, 500)).astype(np.float64))
    assert 10 * 4 + a.nbytes <= cap


def test_dump_outputs_refuses_to_exceed_the_cap(tmp_path):
    with pytest.raises(RuntimeError, match="no room"):
        bench.dump_outputs(str(tmp_path), {"big": torch.zeros(1000)}, cap_bytes=100, sample=500)

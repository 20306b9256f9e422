"""CPU side of the device data route (roko_amd/ops/device_data.py): the
epoch permutation, the whole-group RKW reader, and the config / train()
guards. The kernels are covered by tests/test_gpu_device_data.py."""

import numpy as np
import pytest
import torch

from roko_amd import config as C
from tests.device_data_cases import two_file_dir, write_rkw


def test_epoch_indices_single_rank():
    from roko_amd.ops.device_data import epoch_indices

    a = epoch_indices(1000, 32, seed=5, epoch=1)
    assert a.dtype == np.int32 and a.shape == (992,)
    assert a.min() >= 0 and a.max() < 1000
    assert len(np.unique(a)) == 992
    assert np.array_equal(a, epoch_indices(1000, 32, seed=5, epoch=1))
    assert not np.array_equal(a, epoch_indices(1000, 32, seed=5, epoch=2))


def test_epoch_indices_three_ranks():
    from roko_amd.ops.device_data import epoch_indices

    parts = [epoch_indices(1000, 32, seed=5, epoch=1, rank=r, world=3)
             for r in range(3)]
    assert len({len(p) for p in parts}) == 1
    assert len(parts[0]) > 0 and len(parts[0]) % 32 == 0
    for i in range(3):
        for j in range(i + 1, 3):
            assert not set(parts[i].tolist()) & set(parts[j].tolist())


def test_epoch_indices_too_few_windows():
    from roko_amd.ops.device_data import epoch_indices

    with pytest.raises(ValueError):
        epoch_indices(40, 32, seed=0, epoch=1, rank=0, world=2)


def test_load_rkw_arrays_matches_train_dataset(tmp_path, rng):
    from roko_amd.datasets import TrainDataset
    from roko_amd.ops.device_data import count_rkw_windows, load_rkw_arrays

    d = two_file_dir(tmp_path, rng)
    chunks = list(load_rkw_arrays(d))
    assert [len(x) for x, _ in chunks] == [3, 5, 1]
    x = np.concatenate([c[0] for c in chunks])
    y = np.concatenate([c[1] for c in chunks])
    assert x.dtype == np.uint8 and x.shape == (9, C.WINDOW_ROWS, C.WINDOW_COLS)
    assert y.dtype == np.uint8 and y.shape == (9, C.WINDOW_COLS)
    ds = TrainDataset(d)
    assert len(ds) == 9 == count_rkw_windows(d)
    for i in range(9):
        dx, dy = ds[i]
        assert torch.equal(dx.to(torch.uint8), torch.from_numpy(x[i]))
        assert torch.equal(dy.to(torch.uint8), torch.from_numpy(y[i]))

    inf = write_rkw(str(tmp_path / "inf.rkw"), [2], rng, inference=True)
    with pytest.raises(ValueError, match="inference file"):
        load_rkw_arrays(inf)


def test_train_config_and_cpu_guard(tmp_path, rng):
    from roko_amd.config import TrainConfig
    from roko_amd.train import train

    assert TrainConfig().data == "host"
    with pytest.raises(ValueError):
        TrainConfig(data="bogus")
    path = write_rkw(str(tmp_path / "t.rkw"), [4], rng)
    with pytest.raises(ValueError, match="data='host'"):
        train(path, str(tmp_path / "out"), cfg=TrainConfig(data="device"),
              device=torch.device("cpu"))

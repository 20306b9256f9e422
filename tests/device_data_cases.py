"""Synthetic training RKW files shared by tests/test_device_data.py and
tests/test_gpu_device_data.py."""

import numpy as np

from roko_amd import config as C
from roko_amd.rkdata import RkwWriter


def write_rkw(path, sizes, rng, inference=False):
    """One RKW file with a group per entry of `sizes`, random windows."""
    with RkwWriter(path, inference=inference) as w:
        for gi, n in enumerate(sizes):
            pos = np.zeros((n, C.WINDOW_COLS, 2), dtype=np.int32)
            pos[..., 0] = np.arange(C.WINDOW_COLS)[None, :] + 30 * gi
            x = rng.integers(0, C.NUM_BASE_IDS,
                             (n, C.WINDOW_ROWS, C.WINDOW_COLS), dtype=np.uint8)
            y = None if inference else rng.integers(
                0, C.NUM_CLASSES, (n, C.WINDOW_COLS), dtype=np.uint8)
            w.store("c1", 30 * gi, 30 * gi + C.WINDOW_COLS, pos, x, y)
        w.write_contigs([("c1", "A" * 400)])
    return path


def two_file_dir(tmp_path, rng):
    """Groups of 3 and 5 windows in one file, 1 in the other; the file names
    sort against creation order."""
    d = tmp_path / "set"
    d.mkdir()
    write_rkw(str(d / "b.rkw"), [1], rng)
    write_rkw(str(d / "a.rkw"), [3, 5], rng)
    return str(d)

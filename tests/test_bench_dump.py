"""CPU: bench.py's --dump-outputs writer (dump_outputs): float32 / float64 files, and a fixed seeded sample of the elements
when the arrays exceed the size limit."""
import numpy as np
import torch

import bench


def test_dump_outputs_dtypes(tmp_path):
    bench.dump_outputs(str(tmp_path), {"a": torch.arange(6, dtype=torch.float16).reshape(2, 3), "b": np.float64(2.5),
                                       "c": torch.ones(4, dtype=torch.int32)})
    a, b, c = (np.load(tmp_path / f"{n}.npy") for n in "abc")
    assert a.dtype == np.float32 and a.shape == (2, 3) and a[1, 2] == 5.0
    assert b.dtype == np.float64 and b == 2.5
    assert c.dtype == np.float32 and (c == 1).all()


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4000)
    big = torch.arange(10000, dtype=torch.float32)
    small = torch.arange(10, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "1"), {"big": big, "small": small})
    bench.dump_outputs(str(tmp_path / "2"), {"big": big + 1, "small": small})
    b1, s1 = np.load(tmp_path / "1" / "big.npy"), np.load(tmp_path / "1" / "small.npy")
    b2 = np.load(tmp_path / "2" / "big.npy")
    assert b1.nbytes + s1.nbytes <= 4000 and b1.size == 500 and (s1 == small.numpy()).all()
    assert (np.diff(b1) > 0).all() and (b1 == np.floor(b1)).all()      # the elements at sorted distinct flat indices
    assert (b2 == b1 + 1).all()                                          # the same indices every time

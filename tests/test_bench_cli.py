"""bench.py's command line without a GPU: a plain run asks for the headline step only (--full adds the context sections), and
--dump-outputs writes each output as a float32 .npy file."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_is_lean_by_default():
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = b.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_float32_npy(tmp_path):
    b = _bench()
    rgb = torch.rand(5, 3, dtype=torch.float64)
    b.dump_outputs(str(tmp_path / "d"), {"loss": torch.tensor([0.25]), "comp_rgb": rgb})
    assert sorted(os.listdir(tmp_path / "d")) == ["comp_rgb.npy", "loss.npy"]
    loss, got = np.load(tmp_path / "d" / "loss.npy"), np.load(tmp_path / "d" / "comp_rgb.npy")
    assert loss.dtype == np.float32 and loss.tolist() == [0.25]
    assert got.dtype == np.float32 and got.shape == (5, 3) and np.array_equal(got, rgb.float().numpy())

"""CPU: bench.py's command line and result files -- a plain run is the default, --full is an option, and --dump-outputs writes
a fixed, bounded sample of what the timed step returned."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from richsem_amd import workload as W  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    b = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert (b.full, b.dump_outputs) == (True, "out")


def test_headline_line_reports_the_timed_steps():
    args = bench.parse_args(["--steps", "8", "--warmup", "5"])
    line = bench.headline_line(args, 1, 2, "init", False, 0.024, 13)
    assert line["ms_per_step"] == 3.0 and line["value"] == round(2 / 0.003, 3) and line["steps"] == 8
    assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("img/s", True, "f32")
    assert "roofline" not in line and "cpu_baseline" not in line


def test_output_names_follow_the_step():
    names = bench.step_output_names(W.training_step_calls(2))
    assert len(names) == len(set(names)) == 12 + 12 * 3
    assert names[0] == "E0_out" and names[11] == "Dd5_out"
    assert names[12:15] == ["Dd5_grad_value", "Dd5_grad_loc", "Dd5_grad_attn"] and names[-1] == "E0_grad_attn"
    assert len(names) * bench.DUMP_SAMPLE * 4 <= 64 * 2 ** 20      # the whole dump stays within 64 MB


def test_dump_outputs_writes_a_fixed_sample(tmp_path):
    g = torch.Generator().manual_seed(3)
    big, small = torch.randn(4, 50, 3, generator=g), torch.randn(2, 5, generator=g)
    for d in ("a", "b"):
        n = bench.dump_outputs([("big", big), ("small", small.double())], str(tmp_path / d), sample=64)
        assert n == (64 + 10) * 4
    a_big, b_big = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a_big.dtype == np.float32 and a_big.shape == (64,) and np.array_equal(a_big, b_big)
    assert np.isin(a_big, big.numpy().reshape(-1)).all()
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy().reshape(-1))

"""CPU: bench.py's options (no GPU work): a plain run times the steps and nothing else, --full brings back the verifier,
the CPU baseline and the host path, and --dump-outputs writes a fixed, exact sample of SA and LCP."""
import os

import numpy as np
import pytest

import bench


def test_plain_run_leaves_out_the_extras():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    assert a.no_verify and a.no_cpu_baseline and a.no_host_path


def test_full_runs_the_extras_and_keeps_their_switches():
    a = bench.parse_args(["--full"])
    assert not (a.no_verify or a.no_cpu_baseline or a.no_host_path)
    a = bench.parse_args(["--full", "--no-host-path"])
    assert a.no_host_path and not (a.no_verify or a.no_cpu_baseline)
    a = bench.parse_args(["--cpu-full"])                   # forcing the whole-text CPU baseline implies --full
    assert a.full and not a.no_cpu_baseline


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_is_an_exact_fixed_sample(tmp_path):
    import torch
    n = bench.DUMP_SAMPLE + 12345
    g = torch.Generator().manual_seed(5)
    SA = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int32)     # u32 results live in int32 tensors
    LCP = torch.randint(0, 1000, (n,), generator=g, dtype=torch.int32)
    bench.dump_outputs(torch, str(tmp_path / "a"), SA, LCP, 32)
    bench.dump_outputs(torch, str(tmp_path / "b"), SA, LCP, 32)
    size = 0
    for name, src in (("SA", SA), ("LCP", LCP)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
        u = src.numpy().view(np.uint32).astype(np.float64)
        assert np.isin(a, u).all() and a.min() >= 0
        size += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert size <= 64 * 1000 * 1000
    bench.dump_outputs(torch, str(tmp_path / "c"), SA[:1000].to(torch.int64), LCP[:1000].to(torch.int64), 64)
    assert np.array_equal(np.load(tmp_path / "c" / "SA.npy"), SA[:1000].numpy().astype(np.float64))  # short texts: whole arrays

"""CPU: the CLI's --bwt PATH option is refused, before any file is opened, where there is no BWT to write: no path, several GPUs,
a bounded context.  Each refusal names --bwt and its reason, and leaves neither output file behind."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    return os.path.join(ROOT, "caps-sa_amd", "caps_sa")


@pytest.mark.parametrize("extra,reason", [
    (["--bwt"], "path"),                                        # no path at all
    (["--bwt", "--pretty-print"], "path"),                      # an option where the path should be
    (["--bwt", "{bwt}", "--gpus", "2"], "one GPU"),
    (["--gpus", "3", "--bwt", "{bwt}"], "one GPU"),
    (["8", "50", "--bwt", "{bwt}"], "bounded-context"),
    (["0", "7", "--bwt", "{bwt}"], "bounded-context"),
])
def test_cli_refuses_bwt_before_it_writes(exe, tmp_path, extra, reason):
    inp, out, bwt = tmp_path / "in.txt", tmp_path / "out.bin", tmp_path / "out.bwt"
    inp.write_bytes(b">chr\nACGTNACGT\n" * 40)
    args = [a.format(bwt=bwt) for a in extra]
    r = subprocess.run([exe, str(inp), str(out)] + args, capture_output=True, text=True)
    assert r.returncode != 0, r.stderr
    assert "--bwt" in r.stderr and reason in r.stderr, r.stderr
    assert not out.exists() and not bwt.exists(), r.stderr


def test_cli_bwt_with_a_context_that_bounds_nothing_builds_the_bwt(exe, tmp_path):
    """bounded-context >= n is the suffix array itself (src/main.cpp:57): --bwt is not refused for it, and the CLI runs the build WITH
    the BWT -- with a GPU the file appears (u64 n, u64 primary, n bytes); without one the error names caps_sa_hip_build_bwt, the
    entry point the CLI called."""
    import numpy as np
    inp, out, bwt = tmp_path / "in.txt", tmp_path / "out.bin", tmp_path / "out.bwt"
    inp.write_bytes(b"ACGT" * 100)
    r = subprocess.run([exe, str(inp), str(out), "8", "400", "--bwt", str(bwt)], capture_output=True, text=True)
    assert "--bwt:" not in r.stderr, r.stderr
    if r.returncode == 0:
        b = bwt.read_bytes()
        assert len(b) == 16 + 400 and int(np.frombuffer(b[:8], dtype=np.uint64)[0]) == 400, r.stderr
    else:
        assert "caps_sa_hip_build_bwt" in r.stderr and not bwt.exists(), r.stderr


def test_cli_reports_a_missing_input_as_such(exe, tmp_path):
    """--bwt with a bounded context on an input that does not exist: the missing file is reported, not a bounded-context reason."""
    out, bwt = tmp_path / "out.bin", tmp_path / "out.bwt"
    r = subprocess.run([exe, str(tmp_path / "nope.txt"), str(out), "8", "50", "--bwt", str(bwt)], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot open" in r.stderr and "bounded" not in r.stderr, r.stderr
    assert not out.exists() and not bwt.exists()

"""CPU: the CLI's --inverse-bwt IN.bwt OUT.  Every refusal comes before OUT is opened, names --inverse-bwt and leaves no OUT behind;
a valid file without a GPU fails in the library call, whose name the error carries."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    return os.path.join(ROOT, "caps-sa_amd", "caps_sa")


def _bwt_file(path, n, primary, body):
    path.write_bytes(np.array([n, primary], dtype=np.uint64).tobytes() + body)


@pytest.mark.parametrize("case,reason", [
    ("missing", "cannot open"),
    ("short", "shorter than"),
    ("empty", "shorter than"),
    ("long", "after its header"),
    ("truncated", "after its header"),
    ("primary", "primary"),
    ("option", "usage"),
    ("positional", "usage"),
    ("no_out", "usage"),
    ("build_args", "usage"),
])
def test_cli_refuses_before_it_writes(exe, tmp_path, case, reason):
    inp, out = tmp_path / "in.bwt", tmp_path / "out.txt"
    body = b"ACGT" * 10
    _bwt_file(inp, len(body), 3, body)
    args = ["--inverse-bwt", str(inp), str(out)]
    if case == "missing":
        args[1] = str(tmp_path / "nope.bwt")
    elif case == "short":
        inp.write_bytes(b"\x01" * 15)
    elif case == "empty":
        inp.write_bytes(b"")
    elif case == "long":
        _bwt_file(inp, len(body), 3, body + b"A")
    elif case == "truncated":
        _bwt_file(inp, len(body), 3, body[:-1])
    elif case == "primary":
        _bwt_file(inp, len(body), len(body), body)
    elif case == "option":
        args.append("--pretty-print")
    elif case == "positional":
        args.append("8")
    elif case == "no_out":
        args = args[:2]
    elif case == "build_args":
        args = [str(tmp_path / "x.fa"), str(out), "--inverse-bwt", str(inp)]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode != 0, r.stderr
    assert "--inverse-bwt" in r.stderr and reason in r.stderr, r.stderr
    assert not out.exists(), r.stderr


def test_cli_inverse_without_a_gpu_names_the_entry_point(exe, tmp_path):
    """A well-formed file (the BWT of 'AC' * 20): with a GPU the text comes back; without one the error names
    caps_sa_hip_inverse_bwt and OUT is not written."""
    inp, out = tmp_path / "in.bwt", tmp_path / "out.txt"
    body = b"C" * 20 + b"A" * 20
    _bwt_file(inp, len(body), 19, body)
    expect = b"AC" * 20
    r = subprocess.run([exe, "--inverse-bwt", str(inp), str(out)], capture_output=True, text=True)
    if r.returncode == 0:
        assert out.read_bytes() == expect
    else:
        assert "caps_sa_hip_inverse_bwt" in r.stderr and not out.exists(), r.stderr


def test_cli_empty_text_needs_no_gpu(exe, tmp_path):
    """n = 0: nothing to invert -- an empty OUT, whatever primary says."""
    inp, out = tmp_path / "in.bwt", tmp_path / "out.txt"
    _bwt_file(inp, 0, 5, b"")
    r = subprocess.run([exe, "--inverse-bwt", str(inp), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == b""

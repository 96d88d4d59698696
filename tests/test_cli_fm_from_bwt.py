"""CPU: the CLI's --fm-from-bwt IN.bwt OUT.fm [--fm-sample S].  Every refusal comes before OUT is opened, names the option at fault
and leaves no OUT behind; a valid file without a GPU fails in the library call, whose name the error carries."""
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
    ("sample_in_front", "usage"),
    ("sample_without_value", "usage"),
])
def test_cli_refuses_before_it_writes(exe, tmp_path, case, reason):
    inp, out = tmp_path / "in.bwt", tmp_path / "out.fm"
    body = b"ACGT" * 10
    _bwt_file(inp, len(body), 3, body)
    args = ["--fm-from-bwt", str(inp), str(out)]
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
        args = [str(tmp_path / "x.fa"), str(out), "--fm-from-bwt", str(inp)]
    elif case == "sample_in_front":
        args = ["--fm-sample", "32"] + args
    elif case == "sample_without_value":
        args.append("--fm-sample")
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode != 0, r.stderr
    assert "--fm-from-bwt" in r.stderr and reason in r.stderr, r.stderr
    assert not out.exists(), r.stderr


@pytest.mark.parametrize("value", ["0", "3", "2048", "many", "-32", ""])
def test_cli_refuses_a_bad_sample_distance(exe, tmp_path, value):
    inp, out = tmp_path / "in.bwt", tmp_path / "out.fm"
    body = b"C" * 20 + b"A" * 20
    _bwt_file(inp, len(body), 19, body)
    r = subprocess.run([exe, "--fm-from-bwt", str(inp), str(out), "--fm-sample", value], capture_output=True, text=True)
    assert r.returncode != 0, r.stderr
    assert "--fm-sample" in r.stderr and "power of two" in r.stderr, r.stderr
    assert not out.exists(), r.stderr


def test_cli_without_a_gpu_names_the_entry_point(exe, tmp_path):
    """A well-formed file (the BWT of 'AC' * 20): with a GPU the index is written, an FM blob of n = 40 with samples every 4
    positions; without one the error names caps_sa_hip_fm_build_from_bwt and OUT is not written."""
    inp, out = tmp_path / "in.bwt", tmp_path / "out.fm"
    body = b"C" * 20 + b"A" * 20
    _bwt_file(inp, len(body), 19, body)
    r = subprocess.run([exe, "--fm-from-bwt", str(inp), str(out), "--fm-sample", "4"], capture_output=True, text=True)
    if r.returncode == 0:
        blob = out.read_bytes()
        hdr = np.frombuffer(blob[:256], dtype=np.uint64)
        assert blob[:8] == b"CAPSFMI1" and int(hdr[2]) == 40 and int(hdr[3]) == 19 and int(hdr[12]) == 4 and int(hdr[18]) == len(blob)
    else:
        assert "caps_sa_hip_fm_build_from_bwt" in r.stderr and not out.exists(), r.stderr


def test_usage_lists_the_mode(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0 and "--fm-from-bwt IN.bwt OUT.fm [--fm-sample S]" in r.stderr, r.stderr

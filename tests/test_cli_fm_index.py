"""CPU: the CLI's --fm-index PATH [--fm-sample S] and --fm-search INDEX PATTERNS [--locate K].  Every refusal comes before any
file is opened or written and names its option; a wrong index file is refused by the library's header check, which needs no GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    return os.path.join(ROOT, "caps-sa_amd", "caps_sa")


@pytest.mark.parametrize("extra,reason", [
    (["--fm-index"], "--fm-index: missing output path"),
    (["--fm-index", "--pretty-print"], "--fm-index: missing output path"),
    (["--fm-index", "X", "--gpus", "2"], "--fm-index: the index is built on one GPU"),
    (["8", "16", "--fm-index", "X"], "--fm-index: a bounded-context order"),
    (["--fm-index", "X", "--fm-sample", "3"], "--fm-sample: a power of two"),
    (["--fm-index", "X", "--fm-sample", "2048"], "--fm-sample: a power of two"),
    (["--fm-index", "X", "--fm-sample"], "--fm-sample: a power of two"),
    (["--fm-sample", "32"], "--fm-sample: only with --fm-index"),
    (["--fm-index", "X", "--locate", "5"], "--locate: only with --fm-search"),
])
def test_fm_index_refused_before_any_file_is_written(exe, tmp_path, extra, reason):
    inp, out, fm = tmp_path / "in.fa", tmp_path / "out.bin", tmp_path / "x.fm"
    inp.write_bytes(b"ACGT" * 100)
    extra = [str(fm) if a == "X" else a for a in extra]
    r = subprocess.run([exe, str(inp), str(out)] + extra, capture_output=True, text=True)
    assert r.returncode != 0 and reason in r.stderr, r.stderr
    assert not out.exists() and not fm.exists()


def test_usage_names_the_options(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0
    assert "--fm-index PATH" in r.stderr and "--fm-sample S" in r.stderr and "--fm-search INDEX PATTERNS [--locate K]" in r.stderr
    assert "--bwt PATH" in r.stderr and "--inverse-bwt IN.bwt OUT" in r.stderr     # (what was there stays)


@pytest.mark.parametrize("args", [
    ["--fm-search"],
    ["--fm-search", "I"],
    ["--fm-search", "I", "P", "--locate"],
    ["--fm-search", "I", "P", "--locate", "x"],
    ["--fm-search", "I", "P", "--locate", "0"],
    ["--fm-search", "I", "P", "--pretty-print"],
    ["--fm-search", "I", "P", "--locate", "5", "7"],
    ["--fm-search", "--locate", "5", "I", "P"],
    ["in.fa", "out.bin", "--fm-search", "I", "P"],
])
def test_fm_search_usage(exe, tmp_path, args):
    idx, pats = tmp_path / "i.fm", tmp_path / "p.txt"
    idx.write_bytes(b"\0" * 300)
    pats.write_bytes(b"ACGT\n")
    args = [str(idx) if a == "I" else str(pats) if a == "P" else a for a in args]
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "--fm-search: usage" in r.stderr, r.stderr
    assert r.stdout == ""


@pytest.mark.parametrize("case,reason", [
    ("missing_index", "cannot open"),
    ("missing_patterns", "cannot open"),
    ("not_an_index", "wrong magic"),
    ("short", "smaller than an FM-index header"),
    ("empty", "null index"),
])
def test_fm_search_refuses_a_wrong_index_without_a_gpu(exe, tmp_path, case, reason):
    idx, pats = tmp_path / "i.fm", tmp_path / "p.txt"
    pats.write_bytes(b"ACGT\nAC\n")
    if case == "not_an_index":
        idx.write_bytes(np.arange(4096, dtype=np.uint8).tobytes())
    elif case == "short":
        idx.write_bytes(b"CAPSFMI1" + b"\0" * 40)
    elif case == "empty":
        idx.write_bytes(b"")
    elif case == "missing_patterns":
        idx.write_bytes(b"\0" * 300)
        pats.unlink()
    r = subprocess.run([exe, "--fm-search", str(idx), str(pats), "--locate", "3"], capture_output=True, text=True)
    assert r.returncode != 0 and reason in r.stderr, r.stderr
    assert r.stdout == ""

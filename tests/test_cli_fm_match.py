"""CPU: the CLI's --fm-mems INDEX PATTERNS [--min-len L].  Every refusal comes before anything is printed and names the option; a
wrong index file is refused by the library's header check, which needs no GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    return os.path.join(ROOT, "caps-sa_amd", "caps_sa")


def test_usage_names_the_option(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0 and "--fm-mems INDEX PATTERNS [--min-len L]" in r.stderr
    assert "--fm-search INDEX PATTERNS [--locate K]" in r.stderr and "--fm-extract INDEX RANGES" in r.stderr     # (what was there stays)


@pytest.mark.parametrize("args", [
    ["--fm-mems"],
    ["--fm-mems", "I"],
    ["--fm-mems", "I", "P", "--min-len"],
    ["--fm-mems", "I", "P", "--min-len", "x"],
    ["--fm-mems", "I", "P", "--min-len", "0"],
    ["--fm-mems", "I", "P", "--min-len", "-3"],
    ["--fm-mems", "I", "P", "--min-len", "4294967296"],
    ["--fm-mems", "I", "P", "--locate", "5"],
    ["--fm-mems", "I", "P", "--pretty-print"],
    ["--fm-mems", "I", "P", "--min-len", "5", "7"],
    ["--fm-mems", "--min-len", "5", "I", "P"],
    ["in.fa", "out.bin", "--fm-mems", "I", "P"],
])
def test_fm_mems_usage(exe, tmp_path, args):
    idx, pats = tmp_path / "i.fm", tmp_path / "p.txt"
    idx.write_bytes(b"\0" * 300)
    pats.write_bytes(b"ACGT\n")
    args = [str(idx) if a == "I" else str(pats) if a == "P" else a for a in args]
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "--fm-mems: usage" in r.stderr, r.stderr
    assert r.stdout == ""


def test_min_len_alone_is_refused(exe, tmp_path):
    inp, out = tmp_path / "in.fa", tmp_path / "out.bin"
    inp.write_bytes(b"ACGT" * 100)
    r = subprocess.run([exe, str(inp), str(out), "--min-len", "5"], capture_output=True, text=True)
    assert r.returncode != 0 and "--min-len: only with --fm-mems" in r.stderr and not out.exists()


@pytest.mark.parametrize("case,reason", [
    ("missing_index", "cannot open"),
    ("missing_patterns", "cannot open"),
    ("not_an_index", "wrong magic"),
    ("short", "smaller than an FM-index header"),
    ("empty", "null index"),
    ("bad_header", "FM-index header"),
])
def test_fm_mems_refuses_a_wrong_index_without_a_gpu(exe, tmp_path, case, reason):
    idx, pats = tmp_path / "i.fm", tmp_path / "p.txt"
    pats.write_bytes(b"ACGT\nAC\n")
    if case == "not_an_index":
        idx.write_bytes(np.arange(4096, dtype=np.uint8).tobytes())
    elif case == "short":
        idx.write_bytes(b"CAPSFMI1" + b"\0" * 40)
    elif case == "empty":
        idx.write_bytes(b"")
    elif case == "bad_header":
        h = np.zeros(512, dtype=np.uint64)
        h[0], h[1], h[2], h[4], h[5] = int.from_bytes(b"CAPSFMI1", "little"), 1, 100, 4, 4      # (no section offset fits)
        idx.write_bytes(h.tobytes())
    elif case == "missing_patterns":
        idx.write_bytes(b"\0" * 300)
        pats.unlink()
    r = subprocess.run([exe, "--fm-mems", str(idx), str(pats), "--min-len", "3"], capture_output=True, text=True)
    assert r.returncode != 0 and reason in r.stderr, r.stderr
    assert r.stdout == ""

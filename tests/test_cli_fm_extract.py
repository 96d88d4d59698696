"""CPU: the CLI's --fm-extract INDEX RANGES and --fm-text-sample T.  Every refusal names the option at fault, prints nothing to
stdout and comes before any GPU work; the index files are made with the numpy encoders (fm_reference, fm_extract_reference)."""
import os
import subprocess

import numpy as np
import pytest

import fm_extract_reference as X
import fm_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    return os.path.join(ROOT, "caps-sa_amd", "caps_sa")


@pytest.fixture(scope="module")
def blobs():
    T = np.frombuffer(b"ACGTTGCAAC" * 10, dtype=np.uint8)
    SA = R.naive_sa(T)
    B, primary = R.bwt_of(T, SA)
    v1 = R.encode(B, primary, SA, 4, 4)
    return T, v1, X.add_text_samples(v1, SA, 8), R.encode(B, primary)


@pytest.mark.parametrize("case,reason", [
    ("no_ranges", "usage"),
    ("third_argument", "usage"),
    ("option_behind", "usage"),
    ("option_in_front", "usage"),
    ("option_as_index", "usage"),
    ("with_build_arguments", "usage"),
    ("missing_ranges", "cannot open"),
    ("missing_index", "cannot open"),
    ("one_number", "line 2"),
    ("three_numbers", "line 1"),
    ("negative", "line 1"),
    ("letters", "line 3"),
    ("blank_line", "line 2"),
    ("not_an_index", "not an FM-index"),
    ("short_index", "not an FM-index"),
    ("version_1", "format version 1"),
    ("without_samples", "format version 1"),
    ("past_n", "past the text"),
    ("start_past_n", "past the text"),
    ("huge_start", "past the text"),
])
def test_cli_refuses(exe, tmp_path, blobs, case, reason):
    T, v1, v2, plain = blobs
    index, ranges = tmp_path / "x.fm", tmp_path / "ranges.txt"
    index.write_bytes(v2.tobytes())
    ranges.write_text("0 5\n10 20\n99 1\n")
    args = ["--fm-extract", str(index), str(ranges)]
    if case == "no_ranges":
        args = args[:2]
    elif case == "third_argument":
        args.append("8")
    elif case == "option_behind":
        args += ["--locate", "3"]
    elif case == "option_in_front":
        args = ["--pretty-print"] + args
    elif case == "option_as_index":
        args[1] = "--fm-index"
    elif case == "with_build_arguments":
        args = [str(tmp_path / "in.fa"), str(tmp_path / "out.bin")] + args
    elif case == "missing_ranges":
        args[2] = str(tmp_path / "nope.txt")
    elif case == "missing_index":
        args[1] = str(tmp_path / "nope.fm")
    elif case == "one_number":
        ranges.write_text("0 5\n10\n")
    elif case == "three_numbers":
        ranges.write_text("0 5 7\n")
    elif case == "negative":
        ranges.write_text("0 -5\n")
    elif case == "letters":
        ranges.write_text("0 5\n1 1\nten 2\n")
    elif case == "blank_line":
        ranges.write_text("0 5\n\n1 1\n")
    elif case == "not_an_index":
        index.write_bytes(b"\x00" * 4096)
    elif case == "short_index":
        index.write_bytes(v2.tobytes()[:100])
    elif case == "version_1":
        index.write_bytes(v1.tobytes())
    elif case == "without_samples":
        index.write_bytes(plain.tobytes())
    elif case == "past_n":
        ranges.write_text("0 5\n95 6\n")
    elif case == "start_past_n":
        ranges.write_text("101 0\n")
    elif case == "huge_start":
        ranges.write_text("9999999999999999999 1\n")
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode != 0, r.stderr
    assert "--fm-extract" in r.stderr and reason in r.stderr, r.stderr
    assert r.stdout == "", r.stdout


def test_cli_extract_without_a_gpu_names_the_entry_point(exe, tmp_path, blobs):
    """Well-formed arguments: with a GPU the lines are the text's; without one the error names caps_sa_hip_fm_extract."""
    T, v1, v2, plain = blobs
    index, ranges = tmp_path / "x.fm", tmp_path / "ranges.txt"
    index.write_bytes(v2.tobytes())
    ranges.write_text("0 5\n10 20\n99 1\n100 0\r\n7 0")
    r = subprocess.run([exe, "--fm-extract", str(index), str(ranges)], capture_output=True, text=True)
    if r.returncode == 0:
        tb = T.tobytes().decode()
        assert r.stdout == "".join(x + "\n" for x in (tb[0:5], tb[10:30], tb[99:100], "", "")), r.stdout
    else:
        assert "caps_sa_hip_fm_extract" in r.stderr and r.stdout == "", r.stderr


@pytest.mark.parametrize("args,reason", [
    (["in.fa", "out.bin", "--fm-text-sample", "64"], "only with --fm-index"),
    (["in.fa", "out.bin", "--fm-index", "x.fm", "--fm-text-sample"], "power of two"),
    (["in.fa", "out.bin", "--fm-index", "x.fm", "--fm-text-sample", "48"], "power of two"),
    (["in.fa", "out.bin", "--fm-index", "x.fm", "--fm-text-sample", "2048"], "power of two"),
    (["in.fa", "out.bin", "--fm-index", "x.fm", "--fm-text-sample", "0"], "power of two"),
    (["in.fa", "out.bin", "--fm-index", "x.fm", "--fm-text-sample", "16"], "--fm-sample is 32"),
    (["in.fa", "out.bin", "--fm-index", "x.fm", "--fm-text-sample", "64", "--fm-sample", "128"], "--fm-sample is 128"),
    (["--fm-search", "x.fm", "pats.txt", "--fm-text-sample", "64"], "usage"),
    (["--inverse-bwt", "x.bwt", "out", "--fm-text-sample", "64"], "usage"),
])
def test_cli_refuses_a_text_sample_out_of_place(exe, tmp_path, args, reason):
    """Before any file is opened: the input does not exist and no output appears."""
    r = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and reason in r.stderr, r.stderr
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("extra,reason", [
    (["--fm-text-sample"], "usage"),
    (["--fm-text-sample", "64", "--fm-text-sample", "64"], "usage"),
    (["--fm-text-sample", "64", "--fm-sample", "32", "8"], "usage"),
    (["--fm-text-sample", "48"], "power of two"),
    (["--fm-text-sample", "2048"], "power of two"),
    (["--fm-text-sample", "16"], "--fm-sample is 32"),
    (["--fm-text-sample", "4", "--fm-sample", "8"], "--fm-sample is 8"),
    (["--fm-sample", "8", "--fm-text-sample", "4"], "--fm-sample is 8"),
])
def test_cli_from_bwt_refuses_a_bad_text_sample(exe, tmp_path, extra, reason):
    inp, out = tmp_path / "in.bwt", tmp_path / "out.fm"
    body = b"C" * 20 + b"A" * 20
    inp.write_bytes(np.array([len(body), 19], dtype=np.uint64).tobytes() + body)
    r = subprocess.run([exe, "--fm-from-bwt", str(inp), str(out)] + extra, capture_output=True, text=True)
    assert r.returncode != 0 and reason in r.stderr, r.stderr
    assert "--fm-from-bwt" in r.stderr or "--fm-text-sample" in r.stderr
    assert not out.exists()


def test_usage_lists_the_modes(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode != 0 and "--fm-extract INDEX RANGES" in r.stderr and "[--fm-text-sample T]" in r.stderr, r.stderr

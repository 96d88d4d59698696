"""CPU: the CLI's --raw build line and the wide FM-index behind --fm-search / --fm-mems / --fm-extract, end to end through the CLI's
own source over the host emulation (tests/emul/emul_cli.cpp).  Everything is compared with the naive suffix array and the numpy
encoders of the two blob formats; the run without --raw is pinned to the remapped text's SA / LCP dump, BWT file and narrow blob."""
import os
import subprocess

import numpy as np
import pytest

import fm_match_reference as M
import fm_reference as R
import fm_wide_reference as W
from emul_util import EMUL_DIR, ROOT

TIMEOUT = 120


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "libcaps_sa_emul.so"])
    out = str(tmp_path_factory.mktemp("emul_cli") / "caps_sa_emul")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", out, os.path.join(EMUL_DIR, "emul_cli.cpp"), "-L" + EMUL_DIR,
                           "-lcaps_sa_emul", "-Wl,-rpath," + EMUL_DIR, "-pthread"])
    return out


def run(cli, *args, cwd=None):
    return subprocess.run([cli] + [str(a) for a in args], capture_output=True, cwd=cwd, timeout=TIMEOUT)


def make_text():
    """701 bytes over 9 letters: ACGT, N, lower case (which the remap folds and --raw must not), a newline and a byte >= 0x80."""
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGTNan\n\xe9", dtype=np.uint8)
    T = letters[rng.choice(letters.size, size=701, p=[.2, .2, .2, .2, .08, .04, .04, .02, .02])].copy()
    T[:9] = letters                                            # every letter occurs
    return T


def remap(b):
    """The CLI's byte remap (toupper in the C locale, then lookup[(c & 6) >> 1])."""
    b = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    low = (b >= ord("a")) & (b <= ord("z"))
    b[low] -= 32
    return np.frombuffer(b"ACTG", dtype=np.uint8)[(b & 6) >> 1]


def dump_of(T, SA):
    return np.uint64(T.size).tobytes() + SA.astype("<u4").tobytes() + R.naive_lcp(T, SA).astype("<u4").tobytes()


def bwt_file_of(T, SA):
    B, primary = R.bwt_of(T, SA)
    return np.array([T.size, primary], dtype="<u8").tobytes() + B.tobytes(), B, primary


PATTERN_LINES = [b"N", b"n", b"a", b"ACG", b"NN", b"GTNA", b"\xe9", b"\xe9A", b"X", b"ACXG", b"", b"TTT\r", b"acgt", b"CANG", b"AnNa\xe9"]


def expected_search(T, SA, lines, k):
    txt = M.Text(T, SA)
    out = []
    for p in lines:
        first, count = (0, T.size) if not p else txt.interval(p)
        out.append(" ".join([str(count)] + [str(int(x)) for x in SA[first:first + min(count, k)]]))
    return ("\n".join(out) + "\n").encode()


def expected_mems(T, SA, lines, min_len):
    txt = M.Text(T, SA)
    out = []
    for p in lines:
        ms = txt.mems(p, min_len) if p else []
        out.append(" ".join([str(len(ms))] + ["%d:%d:%d" % (s, l, c) for s, l, f, c in ms]))
    return ("\n".join(out) + "\n").encode()


@pytest.fixture(scope="module")
def built(cli, tmp_path_factory):
    """One --raw run and one run without it over the same input file."""
    d = tmp_path_factory.mktemp("wide_cli")
    T = make_text()
    (d / "in.txt").write_bytes(T.tobytes())
    (d / "p.txt").write_bytes(b"\n".join(PATTERN_LINES) + b"\n")
    r = run(cli, d / "in.txt", d / "raw.sa", "--raw", "--bwt", d / "raw.bwt", "--fm-index", d / "raw.fm", "--fm-sample", "4")
    assert r.returncode == 0, r.stderr
    r2 = run(cli, d / "in.txt", d / "std.sa", "--bwt", d / "std.bwt", "--fm-index", d / "std.fm", "--fm-sample", "4")
    assert r2.returncode == 0, r2.stderr
    return d, T, r, r2


def test_raw_builds_the_text_as_given(built):
    d, T, r, _ = built
    SA = R.naive_sa(T)
    assert (d / "raw.sa").read_bytes() == dump_of(T, SA)
    bwt_bytes, B, primary = bwt_file_of(T, SA)
    assert (d / "raw.bwt").read_bytes() == bwt_bytes
    blob = (d / "raw.fm").read_bytes()
    assert blob[:8] == b"CAPSFMW1"
    assert blob == W.encode(B, primary, SA, 4, 4).tobytes()
    assert b"wide format, 9 letters" in r.stderr


def test_search_on_a_wide_index_takes_the_lines_as_bytes(cli, built):
    d, T, _, _ = built
    SA = R.naive_sa(T)
    r = run(cli, "--fm-search", d / "raw.fm", d / "p.txt", "--locate", "1000")
    assert r.returncode == 0, r.stderr
    lines = [p.rstrip(b"\r") for p in PATTERN_LINES]
    assert r.stdout == expected_search(T, SA, lines, 1000)
    got = r.stdout.split(b"\n")
    tb = T.tobytes()
    assert int(got[0].split()[0]) == tb.count(b"N") > 0 and int(got[1].split()[0]) == tb.count(b"n") > 0      # neither folded nor remapped
    assert got[8] == b"0" and got[9] == b"0"                   # a byte that is no letter
    r = run(cli, "--fm-search", d / "raw.fm", d / "p.txt")
    assert r.returncode == 0 and r.stdout == expected_search(T, SA, lines, 0)


def test_mems_on_a_wide_index_takes_the_lines_as_bytes(cli, built):
    d, T, _, _ = built
    SA = R.naive_sa(T)
    lines = [p.rstrip(b"\r") for p in PATTERN_LINES]
    for min_len in (1, 3):
        r = run(cli, "--fm-mems", d / "raw.fm", d / "p.txt", "--min-len", min_len)
        assert r.returncode == 0, r.stderr
        assert r.stdout == expected_mems(T, SA, lines, min_len)


def test_without_raw_nothing_changes(cli, built):
    """The reference's contract: the remapped text's SA / LCP dump and BWT file, the narrow blob, and remapped pattern lines."""
    d, T, _, r2 = built
    Tm = remap(T.tobytes())
    SA = R.naive_sa(Tm)
    assert (d / "std.sa").read_bytes() == dump_of(Tm, SA)
    bwt_bytes, B, primary = bwt_file_of(Tm, SA)
    assert (d / "std.bwt").read_bytes() == bwt_bytes
    blob = (d / "std.fm").read_bytes()
    assert blob[:8] == b"CAPSFMI1" and blob == R.encode(B, primary, SA, 4, 4).tobytes()
    assert b"wide" not in r2.stderr and b"FM-index: %d bytes, SA samples every 4 positions.\n" % len(blob) in r2.stderr
    lines = [remap(p.rstrip(b"\r")).tobytes() for p in PATTERN_LINES]
    r = run(cli, "--fm-search", d / "std.fm", d / "p.txt", "--locate", "7")
    assert r.returncode == 0 and r.stdout == expected_search(Tm, SA, lines, 7)
    r = run(cli, "--fm-mems", d / "std.fm", d / "p.txt", "--min-len", "2")
    assert r.returncode == 0 and r.stdout == expected_mems(Tm, SA, lines, 2)
    # and a narrow index with text samples still extracts
    r = run(cli, d / "in.txt", d / "std2.sa", "--fm-index", d / "std2.fm", "--fm-sample", "4", "--fm-text-sample", "8")
    assert r.returncode == 0, r.stderr
    (d / "r.txt").write_bytes(b"0 5\n690 11\n")
    r = run(cli, "--fm-extract", d / "std2.fm", d / "r.txt")
    assert r.returncode == 0 and r.stdout == Tm.tobytes()[:5] + b"\n" + Tm.tobytes()[690:701] + b"\n"


def test_extract_refuses_a_wide_index(cli, built):
    d, _, _, _ = built
    (d / "r.txt").write_bytes(b"0 5\n")
    r = run(cli, "--fm-extract", d / "raw.fm", d / "r.txt")
    assert r.returncode != 0 and r.stdout == b""
    assert b"--fm-extract" in r.stderr and b"wide FM-index" in r.stderr and b"CAPSFMW1" in r.stderr and b"not built for the wide format" in r.stderr


@pytest.mark.parametrize("extra", [["--fm-index", "F", "--fm-text-sample", "32"], ["--fm-text-sample", "32", "--fm-index", "F"],
                                   ["--fm-index", "F", "--fm-sample", "8", "--fm-text-sample", "8", "--bwt", "B"]])
def test_raw_refuses_text_samples_before_any_file(cli, tmp_path, extra):
    T = make_text()
    (tmp_path / "in.txt").write_bytes(T.tobytes())
    args = [str(tmp_path / "out.fm") if a == "F" else str(tmp_path / "out.bwt") if a == "B" else a for a in extra]
    for order in (["--raw"] + args, args + ["--raw"]):
        r = run(cli, tmp_path / "in.txt", tmp_path / "out.sa", *order)
        assert r.returncode != 0 and r.stdout == b""
        assert b"--fm-text-sample" in r.stderr and b"CAPSFMW1" in r.stderr and b"not built for the wide format" in r.stderr
        assert sorted(os.listdir(tmp_path)) == ["in.txt"]


def test_from_bwt_refuses_a_raw_bwt_and_names_the_wide_build(cli, built, tmp_path):
    d, _, _, _ = built
    r = run(cli, "--fm-from-bwt", d / "raw.bwt", tmp_path / "x.fm")
    assert r.returncode != 0 and b"wide" in r.stderr and not (tmp_path / "x.fm").exists()


@pytest.mark.parametrize("args", [["--fm-search", "I", "P", "--raw"], ["--raw", "--fm-search", "I", "P"], ["--fm-mems", "I", "P", "--raw"],
                                  ["--fm-extract", "I", "P", "--raw"], ["--fm-from-bwt", "I", "P", "--raw"], ["--inverse-bwt", "I", "P", "--raw"]])
def test_raw_belongs_to_the_build_line_only(cli, built, tmp_path, args):
    d, _, _, _ = built
    args = [str(d / "raw.fm") if a == "I" else str(d / "p.txt") if a == "P" else a for a in args]
    r = run(cli, *args, cwd=tmp_path)
    assert r.returncode != 0 and b"usage" in r.stderr and r.stdout == b""
    assert os.listdir(tmp_path) == []


def test_product_cli_refuses_without_a_gpu(built, tmp_path):
    """The shipped binary: the refusals that need no device come out of it as out of the emulation build."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "caps-sa_amd"), "caps_sa"])
    exe = os.path.join(ROOT, "caps-sa_amd", "caps_sa")
    d, T, _, _ = built
    (tmp_path / "r.txt").write_bytes(b"0 5\n")
    r = run(exe, "--fm-extract", d / "raw.fm", tmp_path / "r.txt")
    assert r.returncode != 0 and r.stdout == b"" and b"not built for the wide format" in r.stderr
    r = run(exe, d / "in.txt", tmp_path / "o.sa", "--raw", "--fm-index", tmp_path / "o.fm", "--fm-text-sample", "32")
    assert r.returncode != 0 and b"not built for the wide format" in r.stderr and sorted(os.listdir(tmp_path)) == ["r.txt"]
    r = run(exe)
    assert r.returncode != 0 and b"--raw" in r.stderr

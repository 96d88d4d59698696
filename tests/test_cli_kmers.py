"""CPU: the CLI's --kmers and --kmer-spectrum on the build line, end to end through the CLI's own source over the host emulation
(tests/emul/emul_cli_kmers.cpp).  The two files are compared with kmer_reference (collections.Counter over the remapped text);
every refusal comes with a message and before anything is written; a run without the new flags gives the bytes it gave before."""
import os
import subprocess

import numpy as np
import pytest

import kmer_reference as K
from emul_util import EMUL_DIR
from sa_check import sa_lcp

TIMEOUT = 120


def _build(tmp, src, name):
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "libcaps_sa_emul.so"])
    out = str(tmp / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", out, os.path.join(EMUL_DIR, src), "-L" + EMUL_DIR,
                           "-lcaps_sa_emul", "-Wl,-rpath," + EMUL_DIR, "-pthread"])
    return out


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("emul_cli_kmers"), "emul_cli_kmers.cpp", "caps_sa_emul_kmers")


def run(cli, *args):
    return subprocess.run([cli] + [str(a) for a in args], capture_output=True, timeout=TIMEOUT)


def remap(b):
    """The CLI's byte remap (toupper in the C locale, then lookup[(c & 6) >> 1])."""
    b = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    low = (b >= ord("a")) & (b <= ord("z"))
    b[low] -= 32
    return np.frombuffer(b"ACTG", dtype=np.uint8)[(b & 6) >> 1]


def make_input():
    """A FASTA-like file: two headers, lines of 60 bases with a planted repeat, lower case and N."""
    rng = np.random.default_rng(11)
    seq = rng.choice(np.frombuffer(b"ACGTacgtN", dtype=np.uint8), size=1500, p=[.22, .22, .22, .22, .02, .02, .02, .02, .04])
    seq[900:1200] = seq[100:400]
    body = seq.tobytes()
    lines = [b">chr1 a test"] + [body[a:a + 60] for a in range(0, 780, 60)] + [b">chr2"] + [body[a:a + 60] for a in range(780, 1500, 60)]
    return b"\n".join(lines) + b"\n"


def table_file(T, k, lo=1, hi=0):
    return b"".join(m + b"\t" + str(c).encode() + b"\n" for m, c in K.table(T, k, lo, hi))


def spectrum_file(T, k):
    h = K.spectrum(T, k, 1024)
    return "".join(f"{c} {int(h[c])}\n" for c in range(1, 1025)).encode()


@pytest.fixture(scope="module")
def built(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("kmers_cli")
    raw = make_input()
    (d / "in.fa").write_bytes(raw)
    return d, raw, remap(raw)


def test_table_and_spectrum_files(cli, built):
    d, raw, T = built
    r = run(cli, d / "in.fa", d / "a.sa", "--kmers", 5, d / "k5.tsv", "--kmer-spectrum", 5, d / "s5.txt")
    assert r.returncode == 0, r.stderr
    assert (d / "k5.tsv").read_bytes() == table_file(T, 5)
    assert (d / "s5.txt").read_bytes() == spectrum_file(T, 5)
    SA, LCP = sa_lcp(T, 32)
    assert (d / "a.sa").read_bytes() == np.uint64(T.size).tobytes() + SA.tobytes() + LCP.tobytes()
    # the count filters, another k for the spectrum, k = 31 and a k beyond the text
    r = run(cli, d / "in.fa", d / "b.sa", "--kmers", 12, d / "k12.tsv", "--min-count", 2, "--max-count", 3, "--kmer-spectrum", 31, d / "s31.txt")
    assert r.returncode == 0, r.stderr
    want = table_file(T, 12, 2, 3)
    assert want.count(b"\n") > 10 and (d / "k12.tsv").read_bytes() == want
    assert (d / "s31.txt").read_bytes() == spectrum_file(T, 31)
    r = run(cli, d / "in.fa", d / "c.sa", "--kmers", 31, d / "k31.tsv", "--min-count", 2)
    assert r.returncode == 0 and (d / "k31.tsv").read_bytes() == table_file(T, 31, 2)
    r = run(cli, d / "in.fa", d / "c.sa", "--kmers", T.size + 1, d / "none.tsv", "--kmer-spectrum", T.size + 1, d / "none.txt")
    assert r.returncode == 0 and (d / "none.tsv").read_bytes() == b"" and (d / "none.txt").read_bytes() == spectrum_file(T, T.size + 1)


def test_spectrum_with_raw(cli, built):
    d, raw, _ = built
    Traw = np.frombuffer(raw, dtype=np.uint8)
    r = run(cli, d / "in.fa", d / "raw.sa", "--raw", "--kmer-spectrum", 4, d / "raw_s4.txt")
    assert r.returncode == 0, r.stderr
    assert (d / "raw_s4.txt").read_bytes() == spectrum_file(Traw, 4)


@pytest.mark.parametrize("args, word", [
    (["--kmers", "5", "OUT", "--raw"], b"--raw"),
    (["--kmers", "5", "OUT", "CTX"], b"bounded-context"),
    (["--kmer-spectrum", "5", "OUT", "CTX"], b"bounded-context"),
    (["--min-count", "2"], b"--min-count: only with --kmers"),
    (["--max-count", "2"], b"--max-count: only with --kmers"),
    (["--kmer-spectrum", "5", "OUT", "--min-count", "2"], b"--min-count: only with --kmers"),
    (["--kmers", "5", "OUT", "--min-count", "3", "--max-count", "2"], b"--max-count"),
    (["--kmers", "0", "OUT"], b"--kmers: usage"),
    (["--kmers", "x", "OUT"], b"--kmers: usage"),
    (["--kmers", "5"], b"--kmers: usage"),
    (["--kmers", "5", "--raw"], b"--kmers: usage"),
    (["--kmer-spectrum", "0", "OUT"], b"--kmer-spectrum: usage"),
    (["--kmer-spectrum", "5"], b"--kmer-spectrum: usage"),
    (["--kmers", "5", "OUT", "--min-count", "0"], b"--min-count"),
    (["--kmers", "5", "OUT", "--max-count"], b"--max-count"),
    (["--kmers", "5", "OUT", "--kmers", "6", "OUT"], b"given twice"),
])
def test_refusals_come_before_anything_is_written(cli, built, tmp_path, args, word):
    d, _, _ = built
    out, sa = tmp_path / "out.file", tmp_path / "x.sa"
    ctx = "bounded" in word.decode()
    argv = [str(d / "in.fa"), str(sa)] + (["0", "40"] if ctx else []) + [str(out) if a == "OUT" else a for a in args if a != "CTX"]
    r = run(cli, *argv)
    assert r.returncode != 0 and word in r.stderr, (argv, r.stderr)
    assert not out.exists() and not sa.exists()


def test_a_run_without_the_new_flags_is_unchanged(cli, built, tmp_path_factory):
    """The same bytes from the driver with the k-mer entry points and from the driver as it was (emul_cli.cpp), for the plain dump,
    --pretty-print, --bwt and --fm-index; and the k-mer flags change none of them."""
    d, raw, T = built
    old = _build(tmp_path_factory.mktemp("emul_cli_plain"), "emul_cli.cpp", "caps_sa_emul")
    outs = {}
    for tag, exe in (("new", cli), ("old", old)):
        assert run(exe, d / "in.fa", d / f"{tag}.sa", "--bwt", d / f"{tag}.bwt", "--fm-index", d / f"{tag}.fm").returncode == 0
        assert run(exe, d / "in.fa", d / f"{tag}.txt", "--pretty-print").returncode == 0
        outs[tag] = [(d / f"{tag}.{e}").read_bytes() for e in ("sa", "bwt", "fm", "txt")]
    assert outs["new"] == outs["old"]
    r = run(cli, d / "in.fa", d / "with.sa", "--bwt", d / "with.bwt", "--fm-index", d / "with.fm", "--kmers", 7, d / "k7.tsv")
    assert r.returncode == 0, r.stderr
    assert [(d / f"with.{e}").read_bytes() for e in ("sa", "bwt", "fm")] == outs["new"][:3]
    assert (d / "k7.tsv").read_bytes() == table_file(T, 7)

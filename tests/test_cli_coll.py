"""CPU: the CLI's --docs, --kmer-sharing and --coll-kmers on the build line, end to end through the CLI's own source over the host
emulation (tests/emul/emul_cli_coll.cpp).  Both files are compared with coll_reference (the text definitions on the text as built);
every refusal comes with a message and before anything is written; a run without the flags gives the bytes it gave before, and the
older drivers still build and refuse the flags."""
import numpy as np
import pytest

import coll_reference as R
from test_cli_kmers import _build, make_input, remap, run


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("emul_cli_coll"), "emul_cli_coll.cpp", "caps_sa_emul_coll")


def three_records():
    """Three records behind one another, a 0xFF byte behind each: 150 random bases, a copy with a substitution every 29 bases, and a
    copy of the first with its middle third replaced."""
    rng = np.random.default_rng(9)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)
    A = rng.choice(dna, size=150)
    B = A.copy()
    B[7::29] = dna[(np.searchsorted(dna, B[7::29]) + 1) % 4]
    C = A.copy()
    C[50:100] = rng.choice(dna, size=50)
    t = A.tobytes() + b"\xff" + B.tobytes() + b"\xff" + C.tobytes() + b"\xff"
    return t, [(0, 150), (151, 150), (302, 150)]


def docs_file(docs):
    return "".join(f"{s} {l}\n" for s, l in docs).encode()


def sharing_file(t, k, docs):
    freq, shared = R.text_summary(t, k, docs)
    m = len(docs)
    out = "".join(f"S\t{a}\t{b}\t{int(shared[a, b])}\n" for a in range(m) for b in range(a, m))
    return (out + "".join(f"F\t{c}\t{int(freq[c])}\n" for c in range(1, m + 1))).encode()


def kmers_file(t, k, docs, lo=1, hi=0):
    return b"".join(w + b"\t" + str(occ).encode() + b"\t" + f"{mask:016x}".encode() + b"\n"
                    for w, _, occ, mask in R.text_table(t, k, docs) if R.passes(mask, lo, hi))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("coll_cli")
    t, docs = three_records()
    (d / "three.bin").write_bytes(t)
    (d / "three.docs").write_bytes(docs_file(docs))
    raw = make_input()
    (d / "in.fa").write_bytes(raw)
    (d / "in.docs").write_bytes(b"0 500\n500 0\n620\t300\r\n\n1000 400\n")
    return d, t, docs, raw


def test_the_sharing_file_on_raw_bytes(cli, built):
    d, t, docs, _ = built
    r = run(cli, d / "three.bin", d / "a.sa", "--raw", "--docs", d / "three.docs", "--kmer-sharing", 8, d / "a.sharing")
    assert r.returncode == 0, r.stderr
    want = sharing_file(t, 8, docs)
    assert (d / "a.sharing").read_bytes() == want and want.count(b"\n") == 6 + 3
    freq, shared = R.text_summary(t, 8, docs)
    assert 0 < shared[0, 1] < shared[0, 0] and freq[3] > 0 and freq[1] > 0
    assert f"k-mer sharing: {int(freq.sum())} distinct 8-mers in 3 documents, {int(freq[3])} in all of them.".encode() in r.stderr


def test_both_files_without_raw_on_the_remapped_text(cli, built):
    d, _, _, raw = built
    T = remap(raw).tobytes()
    docs = [(0, 500), (500, 0), (620, 300), (1000, 400)]
    r = run(cli, d / "in.fa", d / "r.sa", "--docs", d / "in.docs", "--kmer-sharing", 6, d / "r.sharing", "--coll-kmers", 6, d / "r.kmers")
    assert r.returncode == 0, r.stderr
    assert (d / "r.sharing").read_bytes() == sharing_file(T, 6, docs)
    want = kmers_file(T, 6, docs)
    assert (d / "r.kmers").read_bytes() == want and want.count(b"\n") > 500
    assert f"collection k-mers: {want.count(10)} 6-mers written.".encode() in r.stderr
    for lo, hi, name in ((3, 0, "core"), (1, 1, "private"), (2, 2, "two")):
        args = ["--min-docs", lo] + (["--max-docs", hi] if hi else [])
        assert run(cli, d / "in.fa", d / "f.sa", "--docs", d / "in.docs", "--coll-kmers", 6, d / f"r.{name}", *args).returncode == 0
        want = kmers_file(T, 6, docs, lo, hi)
        assert (d / f"r.{name}").read_bytes() == want and want.count(b"\n") >= (1 if hi else 0)


@pytest.mark.parametrize("args, word", [
    (["--kmer-sharing", "5", "OUT"], b"--kmer-sharing: needs --docs FILE"),
    (["--coll-kmers", "5", "OUT"], b"--coll-kmers: needs --docs FILE"),
    (["--docs", "DOCS"], b"--docs: only with --kmer-sharing K PATH or --coll-kmers K PATH"),
    (["--docs"], b"--docs: usage"),
    (["--docs", "DOCS", "--docs", "DOCS", "--kmer-sharing", "5", "OUT"], b"given twice"),
    (["--docs", "DOCS", "--kmer-sharing"], b"--kmer-sharing: usage"),
    (["--docs", "DOCS", "--kmer-sharing", "0", "OUT"], b"--kmer-sharing: usage"),
    (["--docs", "DOCS", "--coll-kmers", "x", "OUT"], b"--coll-kmers: usage"),
    (["--docs", "DOCS", "--coll-kmers", "5", "--raw"], b"--coll-kmers: usage"),
    (["--docs", "DOCS", "--coll-kmers", "5", "OUT", "--coll-kmers", "6", "OUT"], b"given twice"),
    (["--docs", "DOCS", "--coll-kmers", "5", "OUT", "--raw"], b"--coll-kmers: the table is lines of text"),
    (["--docs", "DOCS", "--kmer-sharing", "5", "OUT", "--min-docs", "2"], b"--min-docs: only with --coll-kmers"),
    (["--docs", "DOCS", "--kmer-sharing", "5", "OUT", "--max-docs", "2"], b"--max-docs: only with --coll-kmers"),
    (["--min-docs", "2"], b"--min-docs: only with --coll-kmers"),
    (["--docs", "DOCS", "--coll-kmers", "5", "OUT", "--min-docs", "0"], b"--min-docs: a number of documents of at least 1"),
    (["--docs", "DOCS", "--coll-kmers", "5", "OUT", "--min-docs", "3", "--max-docs", "2"], b"--min-docs 3 is above --max-docs 2"),
    (["--docs", "DOCS", "--kmer-sharing", "5", "OUT", "CTX"], b"bounded-context"),
    (["--docs", "DOCS", "--coll-kmers", "5", "OUT", "CTX"], b"bounded-context"),
    (["--docs", "MISSING", "--kmer-sharing", "5", "OUT"], b"--docs: cannot open"),
    (["--docs", "BAD:0 10\n5 x\n", "--kmer-sharing", "5", "OUT"], b"--docs: line 2 is not `start length`"),
    (["--docs", "BAD:0 10\n17\n", "--coll-kmers", "5", "OUT"], b"--docs: line 2 is not `start length`"),
    (["--docs", "BAD:0 10\n9 10\n", "--kmer-sharing", "5", "OUT"], b"--docs: document 1 overlaps or precedes"),
    (["--docs", "BAD:50 10\n0 10\n", "--kmer-sharing", "5", "OUT"], b"--docs: document 1 overlaps or precedes"),
    (["--docs", "BAD:0 10\n100 BEYOND\n", "--kmer-sharing", "5", "OUT"], b"passes the end of the text"),
    (["--docs", "BAD:\n\n", "--kmer-sharing", "5", "OUT"], b"--docs: no document"),
    (["--docs", "BAD:" + "0 0\n" * 65, "--kmer-sharing", "5", "OUT"], b"--docs: more than 64 documents"),
])
def test_refusals_come_before_anything_is_written(cli, built, tmp_path, args, word):
    d = built[0]
    out, sa = tmp_path / "out.file", tmp_path / "x.sa"
    n = (d / "in.fa").stat().st_size
    ctx = "CTX" in args
    argv = [str(d / "in.fa"), str(sa)] + (["0", "40"] if ctx else [])
    for a in args:
        if a == "CTX":
            continue
        if a.startswith("BAD:"):
            (tmp_path / "bad.docs").write_text(a[4:].replace("BEYOND", str(n)))
            a = str(tmp_path / "bad.docs")
        argv.append({"OUT": str(out), "DOCS": str(d / "in.docs"), "MISSING": str(tmp_path / "no.docs")}.get(a, a))
    r = run(cli, *argv)
    assert r.returncode != 0 and word in r.stderr, (argv, r.stderr)
    assert not out.exists() and not sa.exists()


def test_sixty_four_documents_and_the_last_one_ending_at_n(cli, built):
    d, t, _, _ = built
    n = len(t)
    docs = [(j * 7, 7) for j in range(63)] + [(441, n - 441)]
    (d / "many.docs").write_bytes(docs_file(docs))
    r = run(cli, d / "three.bin", d / "m.sa", "--raw", "--docs", d / "many.docs", "--kmer-sharing", 3, d / "m.sharing")
    assert r.returncode == 0, r.stderr
    assert (d / "m.sharing").read_bytes() == sharing_file(t, 3, docs)


def test_older_drivers_refuse_the_flags_and_a_run_without_them_is_unchanged(cli, built, tmp_path_factory):
    """emul_cli_cross.cpp still compiles unchanged and refuses the three flags; the same bytes from the newest and the older driver for the
    plain dump, --pretty-print, --bwt, --fm-index, --kmers, --lz77, --lce-index, --cross-mums and --cross-mems; the new flags change none
    of them."""
    d = built[0]
    older = _build(tmp_path_factory.mktemp("emul_cli_older"), "emul_cli_cross.cpp", "caps_sa_emul_cross")
    for argv in (["--docs", d / "in.docs", "--kmer-sharing", 5, d / "never.out"], ["--docs", d / "in.docs", "--coll-kmers", 5, d / "never.out"],
                 ["--docs", d / "in.docs"]):
        r = run(older, d / "in.fa", d / "never.sa", *argv)
        assert r.returncode != 0 and b": not built into this driver" in r.stderr
        assert not (d / "never.sa").exists() and not (d / "never.out").exists()
    rest = ["--bwt", "{}.bwt", "--fm-index", "{}.fm", "--kmers", 7, "{}.k7", "--lz77", "{}.lz77", "--lce-index", "{}.lce", "--cross-mums", 700,
            "{}.mums", "--cross-mems", 700, "{}.mems"]
    exts = ("sa", "bwt", "fm", "k7", "lz77", "lce", "mums", "mems", "txt", "plain")
    outs = {}
    for tag, exe, more in (("new", cli, []), ("old", older, []),
                           ("with", cli, ["--docs", d / "in.docs", "--kmer-sharing", 6, d / "with.sharing", "--coll-kmers", 6, d / "with.kmers"])):
        argv = [str(d / a.format(tag)) if isinstance(a, str) and "{}" in a else a for a in rest]
        r = run(exe, d / "in.fa", d / f"{tag}.sa", *argv, *more)
        assert r.returncode == 0, r.stderr
        assert run(exe, d / "in.fa", d / f"{tag}.txt", "--pretty-print").returncode == 0
        assert run(exe, d / "in.fa", d / f"{tag}.plain").returncode == 0
        outs[tag] = [(d / f"{tag}.{e}").read_bytes() for e in exts]
    assert outs["new"] == outs["old"] == outs["with"]
    T = remap(built[3]).tobytes()
    docs = [(0, 500), (500, 0), (620, 300), (1000, 400)]
    assert (d / "with.sharing").read_bytes() == sharing_file(T, 6, docs) and (d / "with.kmers").read_bytes() == kmers_file(T, 6, docs)

"""CPU: the CLI's --cross-mums and --cross-mems on the build line, end to end through the CLI's own source over the host emulation
(tests/emul/emul_cli_cross.cpp).  The two files are compared with cross_reference (the text definitions on the text as built) and the
summary line on stderr with its numbers; every refusal comes with a message and before anything is written; a run without the flags
gives the bytes it gave before, and the older drivers still build and refuse the flags."""
import numpy as np
import pytest

import cross_reference as R
from sa_check import sa_lcp
from test_cli_kmers import _build, make_input, remap, run


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("emul_cli_cross"), "emul_cli_cross.cpp", "caps_sa_emul_cross")


def two_sides():
    """A . 0xFF . B: 260 random bases, and a copy with a substitution every 37 bases and a reversed stretch."""
    rng = np.random.default_rng(5)
    A = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=260)
    B = A.copy()
    B[11::37] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), B[11::37]) + 1) % 4]
    B[200:230] = B[200:230][::-1].copy()
    return A.tobytes() + b"\xff" + B.tobytes(), A.size + 1


def lines(records):
    return "".join(f"{a}\t{b}\t{l}\n" for a, b, l in records).encode()


def ordered(t, split, min_len, max_occ):
    """The records of the text definitions, put into the header's order by the ranks of the naive suffix array."""
    SA, LCP, BWT = R.naive_sa_lcp_bwt(t)
    rank = {p: r for r, p in enumerate(SA)}
    if max_occ is None:
        rec, skipped = R.mums(t, split, min_len), 0
        rec.sort(key=lambda x: max(rank[x[0]], rank[x[1]]))
    else:
        rec, skipped = R.mems(t, split, min_len, max_occ)
        rec.sort(key=lambda x: (max(rank[x[0]], rank[x[1]]), -min(rank[x[0]], rank[x[1]])))
    by_rank, summary = R.rank_rule(SA, LCP, BWT, split, min_len, max_occ)
    assert rec == by_rank and summary[:2] == [len(rec), skipped]
    return rec, skipped, summary[2:5]


def summary_line(mode, n, skipped, lcs):
    return f"cross-{mode}: {n} records, {skipped} skipped runs, longest common substring {lcs[0]} at {lcs[1]} and {lcs[2]}.".encode()


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("cross_cli")
    t, split = two_sides()
    (d / "two.bin").write_bytes(t)
    raw = make_input()
    (d / "in.fa").write_bytes(raw)
    return d, t, split, raw


def test_the_two_files_and_the_summary_line_on_raw_bytes(cli, built):
    d, t, split, _ = built
    r = run(cli, d / "two.bin", d / "a.sa", "--raw", "--cross-mums", split, d / "a.mums", "--cross-mems", split, d / "a.mems", "--min-len", 8,
            "--max-occ", 3)
    assert r.returncode == 0, r.stderr
    mums, _, lcs = ordered(t, split, 8, None)
    mems, skipped, _ = ordered(t, split, 8, 3)
    assert len(mums) >= 5 and len(mems) >= len(mums) and lcs[0] >= 30
    assert (d / "a.mums").read_bytes() == lines(mums)
    assert (d / "a.mems").read_bytes() == lines(mems)
    assert summary_line("mums", len(mums), 0, lcs) in r.stderr and summary_line("mems", len(mems), skipped, lcs) in r.stderr
    best, at = R.lcs(t, split)
    assert best == lcs[0] and (lcs[1], lcs[2]) in at
    T = np.frombuffer(t, dtype=np.uint8)
    SA, LCP = sa_lcp(T, 32)
    assert (d / "a.sa").read_bytes() == np.uint64(T.size).tobytes() + SA.tobytes() + LCP.tobytes()
    # the defaults: min_len 1, max_occ 64 -- on their own, and --bwt beside them writes the file it always wrote
    r = run(cli, d / "two.bin", d / "b.sa", "--raw", "--cross-mems", split, d / "b.mems", "--bwt", d / "b.bwt")
    assert r.returncode == 0, r.stderr
    mems1, skipped1, _ = ordered(t, split, 1, 64)
    assert skipped1 == 4 and (d / "b.mems").read_bytes() == lines(mems1)        # (A, C, G and T occur more than 64 times each)
    assert summary_line("mems", len(mems1), 4, lcs) in r.stderr
    assert run(cli, d / "two.bin", d / "c.sa", "--raw", "--bwt", d / "c.bwt").returncode == 0
    assert (d / "b.bwt").read_bytes() == (d / "c.bwt").read_bytes() and (d / "b.sa").read_bytes() == (d / "c.sa").read_bytes()


def test_without_raw_the_remapped_text(cli, built):
    d, _, _, raw = built
    T = remap(raw).tobytes()
    split = 700
    r = run(cli, d / "in.fa", d / "r.sa", "--cross-mums", split, d / "r.mums", "--min-len", 10, "--cross-mems", split, d / "r.mems", "--max-occ", 2)
    assert r.returncode == 0, r.stderr
    SA, LCP = sa_lcp(np.frombuffer(T, dtype=np.uint8), 32)
    BWT = np.frombuffer(T, dtype=np.uint8)[(SA.astype(np.int64) - 1) % len(T)]
    for name, occ in (("r.mums", None), ("r.mems", 2)):
        want, summary = R.rank_rule(SA, LCP, BWT, split, 10, occ)
        assert len(want) >= 1 and (d / name).read_bytes() == lines(want)
        assert summary_line(name[2:], summary[0], summary[1], summary[2:5]) in r.stderr
    # (no separator: a match may run across the boundary -- the planted repeat does; every record still matches on the text)
    for a, b, l in R.rank_rule(SA, LCP, BWT, split, 10, 2)[0]:
        assert a < split <= b and T[a:a + l] == T[b:b + l]


@pytest.mark.parametrize("args, word", [
    (["--cross-mums", "5", "OUT", "CTX"], b"bounded-context"),
    (["--cross-mems", "5", "OUT", "CTX"], b"bounded-context"),
    (["--cross-mums", "BEYOND", "OUT"], b"SPLIT is beyond the text"),
    (["--cross-mems", "BEYOND", "OUT", "--raw"], b"SPLIT is beyond the text"),
    (["--cross-mums"], b"--cross-mums: usage"),
    (["--cross-mums", "5"], b"--cross-mums: usage"),
    (["--cross-mems", "x", "OUT"], b"--cross-mems: usage"),
    (["--cross-mums", "5", "--raw"], b"--cross-mums: usage"),
    (["--cross-mums", "5", "OUT", "--cross-mums", "6", "OUT"], b"given twice"),
    (["--cross-mems", "5", "OUT", "--max-occ", "1"], b"--max-occ: a number in 2 .. 64"),
    (["--cross-mems", "5", "OUT", "--max-occ", "65"], b"--max-occ: a number in 2 .. 64"),
    (["--cross-mums", "5", "OUT", "--max-occ", "4"], b"--max-occ: only with --cross-mems"),
    (["--max-occ", "4"], b"--max-occ: only with --cross-mems"),
    (["--cross-mums", "5", "OUT", "--min-len", "0"], b"--min-len: a length of at least 1"),
    (["--cross-mums", "5", "OUT", "--min-len"], b"--min-len: a length of at least 1"),
    (["--cross-mems", "5", "OUT", "--gpus", "2"], b"one GPU"),
    (["--min-len", "3"], b"--min-len: only with --fm-mems"),
])
def test_refusals_come_before_anything_is_written(cli, built, tmp_path, args, word):
    d = built[0]
    out, sa = tmp_path / "out.file", tmp_path / "x.sa"
    n = (d / "in.fa").stat().st_size
    ctx = "CTX" in args
    argv = [str(d / "in.fa"), str(sa)] + (["0", "40"] if ctx else [])
    argv += [str(out) if a == "OUT" else str(n + 1) if a == "BEYOND" else a for a in args if a != "CTX"]
    r = run(cli, *argv)
    assert r.returncode != 0 and word in r.stderr, (argv, r.stderr)
    assert not out.exists() and not sa.exists()


def test_split_at_the_ends_succeeds_with_no_records(cli, built):
    d = built[0]
    n = (d / "two.bin").stat().st_size
    for split in (0, n):
        r = run(cli, d / "two.bin", d / "e.sa", "--raw", "--cross-mums", split, d / "e.mums", "--cross-mems", split, d / "e.mems")
        assert r.returncode == 0, r.stderr
        assert (d / "e.mums").read_bytes() == b"" and (d / "e.mems").read_bytes() == b""
        assert b"cross-mums: 0 records, 0 skipped runs, longest common substring 0 at 0 and 0." in r.stderr


def test_older_drivers_refuse_the_flags_and_a_run_without_them_is_unchanged(cli, built, tmp_path_factory):
    """emul_cli.cpp and emul_cli_lce.cpp still compile unchanged and refuse --cross-mums and --cross-mems; the same bytes from the newest
    and the older drivers for the plain dump, --pretty-print, --bwt, --fm-index, --kmers, --lz77 and --lce-index; the new flags change
    none of them."""
    d = built[0]
    tmp = tmp_path_factory.mktemp("emul_cli_older")
    older = [_build(tmp, "emul_cli.cpp", "caps_sa_emul"), _build(tmp, "emul_cli_lce.cpp", "caps_sa_emul_lce")]
    for exe in older:
        for opt in ("--cross-mums", "--cross-mems"):
            r = run(exe, d / "in.fa", d / "never.sa", opt, 100, d / "never.out")
            assert r.returncode != 0 and opt.encode() + b": not built into this driver" in r.stderr
            assert not (d / "never.sa").exists() and not (d / "never.out").exists()
    outs = {}
    for tag, exe in (("new", cli), ("old", older[0]), ("lce", older[1])):
        assert run(exe, d / "in.fa", d / f"{tag}.sa", "--bwt", d / f"{tag}.bwt", "--fm-index", d / f"{tag}.fm").returncode == 0
        assert run(exe, d / "in.fa", d / f"{tag}.txt", "--pretty-print").returncode == 0
        assert run(exe, d / "in.fa", d / f"{tag}.plain").returncode == 0
        outs[tag] = [(d / f"{tag}.{e}").read_bytes() for e in ("sa", "bwt", "fm", "txt", "plain")]
    assert outs["new"] == outs["old"] == outs["lce"]
    for tag, exe in (("new", cli), ("lce", older[1])):
        r = run(exe, d / "in.fa", d / f"{tag}k.sa", "--kmers", 7, d / f"{tag}.k7", "--lz77", d / f"{tag}.lz77", "--lce-index", d / f"{tag}.lce")
        assert r.returncode == 0, r.stderr
    for e in ("k7", "lz77", "lce"):
        assert (d / f"new.{e}").read_bytes() == (d / f"lce.{e}").read_bytes()
    r = run(cli, d / "in.fa", d / "with.sa", "--bwt", d / "with.bwt", "--fm-index", d / "with.fm", "--lz77", d / "with.lz77", "--kmers", 7,
            d / "with.k7", "--lce-index", d / "with.lce", "--cross-mums", 700, d / "with.mums", "--cross-mems", 700, d / "with.mems")
    assert r.returncode == 0, r.stderr
    assert [(d / f"with.{e}").read_bytes() for e in ("sa", "bwt", "fm")] == outs["new"][:3]
    for e in ("k7", "lz77", "lce"):
        assert (d / f"with.{e}").read_bytes() == (d / f"new.{e}").read_bytes()
    assert (d / "with.mums").exists() and (d / "with.mems").exists()

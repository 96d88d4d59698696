"""CPU: the CLI's --lce-index on the build line and --lce INDEX PAIRS [--mismatches K], end to end through the CLI's own source over
the host emulation (tests/emul/emul_cli_lce.cpp).  The index file is the reference encoder's blob of the text as built, every printed
length is brute force's on that text; every refusal comes with a message and before anything is written; a run without the flags gives
the bytes it gave before, and the older drivers still build and refuse the flags."""
import numpy as np
import pytest

import lce_reference as R
from sa_check import sa_lcp
from test_cli_kmers import _build, make_input, remap, run


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("emul_cli_lce"), "emul_cli_lce.cpp", "caps_sa_emul_lce")


@pytest.fixture(scope="module")
def built(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("lce_cli")
    raw = make_input()
    (d / "in.fa").write_bytes(raw)
    T = remap(raw)
    rs = np.random.RandomState(4)
    pairs = [(int(a), int(b)) for a, b in zip(rs.randint(0, T.size, size=300), rs.randint(0, T.size, size=300))]
    t = T.tobytes()
    again = t.find(t[116:128], 117)                           # the planted repeat: its second copy
    assert again > 0
    pairs += [(0, 0), (T.size - 1, 0), (T.size - 1, T.size - 1), (116, again), (again + 1, 117)]
    (d / "pairs.txt").write_text("".join(f"{a} {b}\n" if k % 2 else f"{a}\t{b}\n" for k, (a, b) in enumerate(pairs)))
    return d, raw, T, pairs


def test_the_round_trip_against_brute_force(cli, built):
    d, raw, T, pairs = built
    r = run(cli, d / "in.fa", d / "a.sa", "--lce-index", d / "a.lce")
    assert r.returncode == 0, r.stderr
    assert b"LCE index" in r.stderr
    SA, LCP = sa_lcp(T, 32)
    assert (d / "a.sa").read_bytes() == np.uint64(T.size).tobytes() + SA.tobytes() + LCP.tobytes()
    assert (d / "a.lce").read_bytes() == R.encode(SA, LCP, 4).tobytes()
    t = T.tobytes()
    for k in (0, 1, 5):
        r = run(cli, "--lce", d / "a.lce", d / "pairs.txt", *(["--mismatches", k] if k else []))
        assert r.returncode == 0, r.stderr
        assert [int(x) for x in r.stdout.split()] == [R.lce_brute(t, a, b, k) for a, b in pairs], k
    assert R.lce_brute(t, *pairs[-2], 0) >= 12 and R.lce_brute(t, *pairs[-2], 5) > R.lce_brute(t, *pairs[-2], 0) + 5      # the planted repeat


def test_raw_bytes_index_the_file_itself(cli, built):
    d, raw, _, pairs = built
    assert run(cli, d / "in.fa", d / "raw.sa", "--raw", "--lce-index", d / "raw.lce").returncode == 0
    r = run(cli, "--lce", d / "raw.lce", d / "pairs.txt", "--mismatches", 2)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split()] == [R.lce_brute(raw, a, b, 2) for a, b in pairs]


@pytest.mark.parametrize("args, word", [
    (["--lce-index", "OUT", "CTX"], b"bounded-context"),
    (["--lce-index"], b"--lce-index: usage"),
    (["--lce-index", "--raw"], b"--lce-index: usage"),
    (["--lce-index", "OUT", "--lce-index", "OUT"], b"given twice"),
    (["--mismatches", "3"], b"--mismatches: only with --lce"),
])
def test_build_line_refusals_come_before_anything_is_written(cli, built, tmp_path, args, word):
    d = built[0]
    out, sa = tmp_path / "out.file", tmp_path / "x.sa"
    ctx = "bounded" in word.decode()
    argv = [str(d / "in.fa"), str(sa)] + (["0", "40"] if ctx else []) + [str(out) if a == "OUT" else a for a in args if a != "CTX"]
    r = run(cli, *argv)
    assert r.returncode != 0 and word in r.stderr, (argv, r.stderr)
    assert not out.exists() and not sa.exists()


def test_query_line_refusals(cli, built, tmp_path):
    d, _, T, _ = built
    assert run(cli, d / "in.fa", d / "q.sa", "--lce-index", d / "q.lce", "--fm-index", d / "q.fm").returncode == 0
    bad = tmp_path / "bad.txt"
    for text, word in (("5 x\n", b"expected \"i j\""), ("5\n", b"expected \"i j\""), (f"3 {T.size}\n", b"past the text")):
        bad.write_text(text)
        r = run(cli, "--lce", d / "q.lce", bad)
        assert r.returncode != 0 and word in r.stderr and r.stdout == b"", (text, r.stderr)
    bad.write_text("")                                        # no pairs: no lines, and no error
    r = run(cli, "--lce", d / "q.lce", bad)
    assert r.returncode == 0 and r.stdout == b""
    ok = tmp_path / "ok.txt"
    ok.write_text("1 2\n")
    for argv, word in (
        (["--lce", d / "q.lce"], b"--lce: usage"),
        (["--lce", d / "q.lce", ok, "--mismatches"], b"--lce: usage"),
        (["--lce", d / "q.lce", ok, "--mismatches", "1025"], b"0 .. 1024"),
        (["--lce", d / "q.lce", ok, "--mismatches", "x"], b"0 .. 1024"),
        (["--lce", d / "q.lce", ok, "--min-len", "3"], b"0 .. 1024"),
        (["--lce", d / "q.fm", ok], b"not an LCE index"),
        (["--lce", tmp_path / "missing.lce", ok], b"cannot open"),
    ):
        r = run(cli, *argv)
        assert r.returncode != 0 and word in r.stderr and r.stdout == b"", (argv, r.stderr)
    blob = bytearray((d / "q.lce").read_bytes())
    blob[6 * 8] ^= 1                                          # a damaged header word: refused by the library
    (tmp_path / "damaged.lce").write_bytes(bytes(blob))
    r = run(cli, "--lce", tmp_path / "damaged.lce", ok)
    assert r.returncode != 0 and b"LCE index header" in r.stderr
    (tmp_path / "short.lce").write_bytes(bytes(blob[:-256]))
    assert run(cli, "--lce", tmp_path / "short.lce", ok).returncode != 0


def test_older_drivers_refuse_the_flags_and_a_run_without_them_is_unchanged(cli, built, tmp_path_factory):
    """emul_cli.cpp, emul_cli_kmers.cpp and emul_cli_lz.cpp still compile unchanged and refuse --lce-index and --lce; the same bytes
    from the newest and the older drivers for the plain dump, --pretty-print, --bwt, --fm-index, --kmers and --lz77; --lce-index
    changes none of them."""
    d = built[0]
    tmp = tmp_path_factory.mktemp("emul_cli_older")
    older = [_build(tmp, "emul_cli.cpp", "caps_sa_emul"), _build(tmp, "emul_cli_kmers.cpp", "caps_sa_emul_kmers"),
             _build(tmp, "emul_cli_lz.cpp", "caps_sa_emul_lz")]
    for exe in older:
        r = run(exe, d / "in.fa", d / "never.sa", "--lce-index", d / "never.lce")
        assert r.returncode != 0 and b"--lce-index: not built into this driver" in r.stderr
        assert not (d / "never.sa").exists() and not (d / "never.lce").exists()
        r = run(exe, "--lce", d / "never.lce", d / "pairs.txt")
        assert r.returncode != 0 and b"--lce: not built into this driver" in r.stderr
    outs = {}
    for tag, exe in (("new", cli), ("old", older[0]), ("lz", older[2])):
        assert run(exe, d / "in.fa", d / f"{tag}.sa", "--bwt", d / f"{tag}.bwt", "--fm-index", d / f"{tag}.fm").returncode == 0
        assert run(exe, d / "in.fa", d / f"{tag}.txt", "--pretty-print").returncode == 0
        outs[tag] = [(d / f"{tag}.{e}").read_bytes() for e in ("sa", "bwt", "fm", "txt")]
    assert outs["new"] == outs["old"] == outs["lz"]
    for tag, exe in (("new", cli), ("lz", older[2])):
        assert run(exe, d / "in.fa", d / f"{tag}k.sa", "--kmers", 7, d / f"{tag}.k7", "--lz77", d / f"{tag}.lz77").returncode == 0
    assert (d / "new.k7").read_bytes() == (d / "lz.k7").read_bytes() and (d / "new.lz77").read_bytes() == (d / "lz.lz77").read_bytes()
    r = run(cli, d / "in.fa", d / "with.sa", "--bwt", d / "with.bwt", "--fm-index", d / "with.fm", "--lz77", d / "with.lz77", "--kmers", 7,
            d / "with.k7", "--lce-index", d / "with.lce")
    assert r.returncode == 0, r.stderr
    assert [(d / f"with.{e}").read_bytes() for e in ("sa", "bwt", "fm")] == outs["new"][:3]
    assert (d / "with.k7").read_bytes() == (d / "new.k7").read_bytes() and (d / "with.lz77").read_bytes() == (d / "new.lz77").read_bytes()
    assert (d / "with.lce").read_bytes()[:8] == b"CAPSLCE1"

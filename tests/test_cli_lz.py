"""CPU: the CLI's --lz77 on the build line, end to end through the CLI's own source over the host emulation
(tests/emul/emul_cli_lz.cpp).  The file alone decodes to the text as built (remapped, or the file's own bytes with --raw) and equals
the reference parse line by line; every refusal comes with a message and before anything is written; a run without the flag gives
the bytes it gave before."""
import numpy as np
import pytest

import lz_reference as R
from sa_check import sa_lcp
from test_cli_kmers import _build, make_input, remap, run


@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("emul_cli_lz"), "emul_cli_lz.cpp", "caps_sa_emul_lz")


@pytest.fixture(scope="module")
def built(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("lz_cli")
    raw = make_input()
    (d / "in.fa").write_bytes(raw)
    return d, raw, remap(raw)


def decode(data: bytes) -> bytes:
    """The text from the file alone."""
    out = bytearray()
    for line in data.decode().splitlines():
        pos, ln, src = (int(x) for x in line.split("\t"))
        assert pos == len(out)
        if ln == 0:
            out.append(src)
        else:
            assert src < pos
            for k in range(ln):
                out.append(out[src + k])
    return bytes(out)


def parse_file(T):
    SA, LCP = sa_lcp(T, 32)
    L, P = R.lpf_stack(SA, LCP)
    t = T.tobytes()
    return "".join(f"{pos}\t0\t{t[pos]}\n" if src == R.LITERAL else f"{pos}\t{ln}\t{src}\n" for pos, ln, src in R.lz_parse(L, P, T.size)).encode()


def test_the_file_decodes_to_the_text(cli, built):
    d, raw, T = built
    r = run(cli, d / "in.fa", d / "a.sa", "--lz77", d / "a.lz")
    assert r.returncode == 0, r.stderr
    data = (d / "a.lz").read_bytes()
    assert decode(data) == T.tobytes()
    assert data == parse_file(T)
    lines = data.decode().splitlines()
    assert sum(1 for x in lines if x.split("\t")[1] == "0") == 4                  # one literal per letter of the remapped text
    assert max(int(x.split("\t")[1]) for x in lines) > 20                          # the planted repeat, cut by the line ends
    SA, LCP = sa_lcp(T, 32)
    assert (d / "a.sa").read_bytes() == np.uint64(T.size).tobytes() + SA.tobytes() + LCP.tobytes()
    assert b"phrases written" in r.stderr


def test_raw_bytes_decode_too(cli, built):
    d, raw, _ = built
    r = run(cli, d / "in.fa", d / "raw.sa", "--raw", "--lz77", d / "raw.lz")
    assert r.returncode == 0, r.stderr
    data = (d / "raw.lz").read_bytes()
    assert decode(data) == raw and data == parse_file(np.frombuffer(raw, dtype=np.uint8))


@pytest.mark.parametrize("args, word", [
    (["--lz77", "OUT", "CTX"], b"bounded-context"),
    (["--lz77"], b"--lz77: usage"),
    (["--lz77", "--raw"], b"--lz77: usage"),
    (["--lz77", "OUT", "--lz77", "OUT"], b"given twice"),
])
def test_refusals_come_before_anything_is_written(cli, built, tmp_path, args, word):
    d, _, _ = built
    out, sa = tmp_path / "out.file", tmp_path / "x.sa"
    ctx = "bounded" in word.decode()
    argv = [str(d / "in.fa"), str(sa)] + (["0", "40"] if ctx else []) + [str(out) if a == "OUT" else a for a in args if a != "CTX"]
    r = run(cli, *argv)
    assert r.returncode != 0 and word in r.stderr, (argv, r.stderr)
    assert not out.exists() and not sa.exists()


def test_drivers_that_predate_the_flag_refuse_it_and_a_run_without_it_is_unchanged(cli, built, tmp_path_factory):
    """emul_cli.cpp and emul_cli_kmers.cpp still compile unchanged and refuse --lz77; the same bytes from all three drivers for the
    plain dump, --pretty-print, --bwt, --fm-index and --kmers; and --lz77 changes none of them."""
    d, raw, T = built
    tmp = tmp_path_factory.mktemp("emul_cli_older")
    plain, kmers = _build(tmp, "emul_cli.cpp", "caps_sa_emul"), _build(tmp, "emul_cli_kmers.cpp", "caps_sa_emul_kmers")
    for exe in (plain, kmers):
        r = run(exe, d / "in.fa", d / "never.sa", "--lz77", d / "never.lz")
        assert r.returncode != 0 and b"--lz77: not built into this driver" in r.stderr
        assert not (d / "never.sa").exists() and not (d / "never.lz").exists()
    outs = {}
    for tag, exe in (("new", cli), ("old", plain), ("mid", kmers)):
        assert run(exe, d / "in.fa", d / f"{tag}.sa", "--bwt", d / f"{tag}.bwt", "--fm-index", d / f"{tag}.fm").returncode == 0
        assert run(exe, d / "in.fa", d / f"{tag}.txt", "--pretty-print").returncode == 0
        outs[tag] = [(d / f"{tag}.{e}").read_bytes() for e in ("sa", "bwt", "fm", "txt")]
    assert outs["new"] == outs["old"] == outs["mid"]
    for tag, exe in (("new", cli), ("mid", kmers)):
        assert run(exe, d / "in.fa", d / f"{tag}k.sa", "--kmers", 7, d / f"{tag}.k7").returncode == 0
    assert (d / "new.k7").read_bytes() == (d / "mid.k7").read_bytes()
    r = run(cli, d / "in.fa", d / "with.sa", "--bwt", d / "with.bwt", "--fm-index", d / "with.fm", "--lz77", d / "with.lz", "--kmers", 7, d / "with.k7")
    assert r.returncode == 0, r.stderr
    assert [(d / f"with.{e}").read_bytes() for e in ("sa", "bwt", "fm")] == outs["new"][:3]
    assert (d / "with.k7").read_bytes() == (d / "new.k7").read_bytes() and decode((d / "with.lz").read_bytes()) == T.tobytes()

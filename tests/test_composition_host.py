"""pss-bam -P without a GPU: composition_lib's restatement of the definition against the rows the unmodified reference wrote
(tests/golden/composition10_set?.txt: the three ties of include/pssbam_hip.h) and against the context rows of the counts
goldens that were committed long before; the width parser and the writer of the composition file in libpssbam_host.so; the
C-ABI symbols of libpssbam_hip.so; the command line's diagnostics."""
import ctypes as C
import json
import re
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import composition_lib as cl
import interior_lib as il
import mismatch_lib as ml
import pssbam_testlib as tl
import site_context_lib as sc

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
W = 10
MIN_LEN = 15


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


@pytest.fixture(scope="module")
def host(pkg):
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_composition_width.restype = C.c_int
    L.pss_parse_composition_width.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.pss_composition_fractions.restype = None
    L.pss_composition_fractions.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    L.pss_write_composition.restype = C.c_int
    L.pss_write_composition.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


@pytest.fixture(scope="module", params=["setA", "setD"])
def dataset(request):
    base = request.param
    contigs = sc.read_fasta(GOLD / f"{base}.fa")
    refs, recs = ml.read_sam(GOLD / f"{base}.sam")
    w, ties = cl.parse_golden((GOLD / f"composition{W}_{base}.txt").read_text())
    assert w == W
    return base, contigs, recs, ties


def rows_of(c5, c3, offsets):
    return {(b, j): [int(x) for x in t[j + W, :4]] for b, t in (("c5", c5), ("c3", c3)) for j in offsets}


# ---- the restatement against the reference's rows ------------------------------------------------------------------------

def test_golden_is_not_vacuous(dataset):
    base, contigs, recs, ties = dataset
    assert set(ties) == {"tie1", "tie2", "tie3"}
    assert set(ties["tie1"]) == {(b, j) for b in ("c5", "c3") for j in (-1, -2)}
    assert set(ties["tie2"]) == {(b, j) for b in ("c5", "c3") for j in range(W)}
    assert set(ties["tie3"]) == {(b, -j) for b in ("c5", "c3") for j in range(3, W + 1)}
    for tie in ties.values():
        for row in tie.values():
            assert sum(row) >= 100 and all(v > 0 for v in row)
    assert ties["tie1"][("c5", -1)] != ties["tie1"][("c3", -1)] and ties["tie3"][("c5", -3)] != ties["tie3"][("c5", -4)]
    assert any(r.flag & 0x10 for r in recs) and any(r.flag & 0x40 for r in recs) and any(r.flag & 0x80 for r in recs)
    assert base != "setA" or any(cl.cls(ch) == 4 for _, t in contigs for ch in t.upper())     # setA holds other letters, setD none


def test_tie1_context_rows(dataset):
    _, contigs, recs, ties = dataset
    c5, c3, n_fwd, n_rev = cl.composition(recs, contigs, W)
    assert rows_of(c5, c3, (-1, -2)) == ties["tie1"] and n_fwd > 100 and n_rev > 100


def test_tie2_inside_rows(dataset):
    """the reference ran on the all-A records with -r 10; the composition is the same before and after that replacement"""
    _, contigs, recs, ties = dataset
    o = replace(tl.PssOpts(), region_len=W)
    c5, c3, _, _ = cl.composition(recs, contigs, W, o)
    assert rows_of(c5, c3, range(W)) == ties["tie2"]
    a5, a3, _, _ = cl.composition(cl.all_a(recs), contigs, W, o)
    assert np.array_equal(a5, c5) and np.array_equal(a3, c3)


def test_tie3_outside_rows(dataset):
    _, contigs, recs, ties = dataset
    letters = cl.fasta_letters(contigs)
    far = cl.far_from_edges(recs, contigs, W, MIN_LEN)
    assert len(far) > 100 and any(r.flag & 0x10 for r in far)
    c5, c3, n_fwd, n_rev = cl.composition(far, contigs, W, replace(tl.PssOpts(), up_ctx=letters, down_ctx=letters))
    assert n_fwd == n_rev > 100                                                  # unpaired, nothing rejected by -U / -D: both tables
    assert rows_of(c5, c3, range(-W, -2)) == ties["tie3"]


def test_shifted_records_move_the_context_row():
    """(the builder itself) context row -2 of the lengthened record is the outside row -j of the original"""
    text = il.clean_contig(400, seed=3)
    for flag in (0, 16):
        r = il.read_on(text, 100, 30, flag=flag)
        for block in ("c5", "c3"):
            for j in (3, 10):
                m = cl.shifted([r], j, block)[0]
                assert m.cigar == [(30 + j - 2, "M")] and len(m.seq) == len(m.qual) == 30 + j - 2
                a = cl.composition([r], {"c": text}, 10)[0 if block == "c5" else 1][10 - j]
                b = cl.composition([m], {"c": text}, 10)[0 if block == "c5" else 1][10 - 2]
                assert np.array_equal(a, b) and a.sum() == 1


MANIFEST = json.loads((GOLD / "manifest.json").read_text())
PSS_CASES = [c for c in MANIFEST["cases"] if c["tool"] == "pss-bam" and c["opts"]["read_group"] is None]


@pytest.mark.parametrize("case", PSS_CASES, ids=[c["prefix"] for c in PSS_CASES])
def test_tie1_against_the_committed_counts_goldens(case):
    """rows w-1 and w-2 of both blocks are the diagonals of the context rows of the reference's counts file, at any options"""
    ds = MANIFEST["datasets"][case["dataset"]]
    contigs = sc.read_fasta(GOLD / ds["fasta"])
    _, recs = ml.read_sam(GOLD / ds["sam"])
    o = tl.PssOpts(**case["opts"])
    fwd, rev = tl.parse_counts_text((GOLD / case["counts"]).read_text())
    want = cl.context_rows(fwd, rev)
    assert sum(sum(v) for v in want.values()) > 40
    for w in (2, 7, 30):
        c5, c3, _, _ = cl.composition(recs, contigs, w, o)
        got = {(b, -k): [int(x) for x in t[w - k, :4]] for b, t in (("c5", c5), ("c3", c3)) for k in (1, 2)}
        assert got == want


def test_restatement_by_hand():
    """strands, the complement, the edges of the contig and reads shorter than the window"""
    text = "ACGTN" + "ACCGGGTTTT" * 3 + "acgtR"                                # 40 letters
    ctg = {"c": text}
    o = tl.PssOpts(region_len=0, up_ctx="ACGTN", down_ctx="ACGTN")                 # (the N next to the read must not reject it)
    fwd_rec = il.read_on(text, 5, 10)                                              # s = 5, L = 10: ACCGGGTTTT
    c5, c3, _, _ = cl.composition([fwd_rec], ctg, 12, o)
    assert [int(np.argmax(c5[12 + j])) for j in range(10)] == [cl.cls(x) for x in "ACCGGGTTTT"]
    assert not c5[12 + 10:].any() and not c3[12 + 10:].any()                      # inside offsets >= L stay empty
    assert [int(np.argmax(c5[12 + j])) for j in (-1, -2, -3, -4, -5)] == [4, 3, 2, 1, 0] and not c5[:12 - 5].any()   # N T G C A, then the edge
    assert [int(np.argmax(c3[12 + j])) for j in range(3)] == [3, 3, 3] and int(np.argmax(c3[12 - 1])) == 0
    rev_rec = replace(fwd_rec, flag=16)
    r5, r3, _, _ = cl.composition([rev_rec], ctg, 12, o)
    assert [int(np.argmax(r5[12 + j])) for j in range(4)] == [0, 0, 0, 0]         # T at the right end, complemented
    assert int(np.argmax(r5[12 - 1])) == 3 and int(np.argmax(r3[12 - 1])) == 4    # A past the right end -> T; N stays other
    assert int(r5.sum()) == int(c3.sum()) and int(r3.sum()) == int(c5.sum())
    n5, n3 = cl.positions_exist([fwd_rec, rev_rec], ctg, 12, o)
    assert list(n5[12:22]) == [2] * 10 and n5[11] == 2 and n5[0] == 1 and n3[0] == 1
    r1 = replace(fwd_rec, flag=0x1 | 0x2 | 0x40, tlen=10)
    r2 = replace(fwd_rec, flag=0x1 | 0x2 | 0x80, tlen=-10)
    a5, a3, nf, nr = cl.composition([r1], ctg, 3, o)
    assert a5.any() and not a3.any() and (nf, nr) == (1, 0)
    a5, a3, nf, nr = cl.composition([r2], ctg, 3, o)
    assert a3.any() and not a5.any() and (nf, nr) == (0, 1)


# ---- parser --------------------------------------------------------------------------------------------------------------

def parse(host, arg: bytes):
    """the value, or the diagnostic (str) of a rejection"""
    err = C.create_string_buffer(200)
    v = host.pss_parse_composition_width(arg, err, len(err))
    if v < 0:
        assert v == -1 and err.value and b"\n" not in err.value, arg
        return err.value.decode()
    return v


@pytest.mark.parametrize("arg,want", [(b"1", 1), (b"2", 2), (b"10", 10), (b"30", 30), (b"007", 7)])
def test_parser_accepts(host, arg, want):
    assert parse(host, arg) == want


@pytest.mark.parametrize("arg", [b"0", b"31", b"-1", b"12x", b"", b"+5", b" 5", b"5 ", b"3.5", b"0x10", b"99999999999999999999"])
def test_parser_rejects_with_a_message(host, arg):
    msg = parse(host, arg)
    assert isinstance(msg, str) and "-P" in msg and "1..30" in msg


def test_parser_diagnostics_name_the_problem(host):
    assert "above 30" in parse(host, b"31") and "below 1" in parse(host, b"0")
    assert "decimal" in parse(host, b"12x") and "needs" in parse(host, b"")


# ---- fractions and writer ------------------------------------------------------------------------------------------------

def test_fractions_leave_other_out_and_are_zero_without_bases(host):
    frac = (C.c_double * 4)()
    host.pss_composition_fractions((C.c_uint64 * 5)(1, 2, 3, 4, 1000), frac)
    assert list(frac) == [1 / 10, 2 / 10, 3 / 10, 4 / 10]
    host.pss_composition_fractions((C.c_uint64 * 5)(0, 0, 0, 0, 7), frac)
    assert list(frac) == [0.0] * 4
    host.pss_composition_fractions((C.c_uint64 * 5)(2 ** 40, 0, 2 ** 40, 0, 0), frac)
    assert list(frac) == [0.5, 0.0, 0.5, 0.0]


def test_write_composition_exact_bytes(host, tmp_path):
    w = 3
    rng = np.random.default_rng(5)
    c5 = rng.integers(0, 1000, size=(2 * w, 5)).astype(np.uint64)
    c3 = rng.integers(0, 1000, size=(2 * w, 5)).astype(np.uint64)
    c5[0] = [0, 0, 0, 0, 9]                                                  # no base at all: the four fractions print as zero
    c3[1] = [2 ** 32 + 5, 1, 2, 3, 4]
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))                  # noqa: E731
    assert host.pss_write_composition(b"the genome.fa", b"in.bam", str(tmp_path / "out").encode(), w, ptr(c5), ptr(c3)) == 0
    text = (tmp_path / "out.pss.composition.txt").read_text()
    row = lambda label, r: f"{label}\t" + "".join(f"{int(x)}\t" for x in r) + "".join(f"{x}\t" for x in cl.fractions(r)) + "\n"   # noqa: E731
    want = ("# reference base composition 3 bases on either side of the ends of the tallied reads, in the read's orientation"
            " (negative: outside the read)\n"
            "# FASTA: the genome.fa\n"
            "# BAM: in.bam\n"
            "### POS A C G T other fA fC fG fT\n"
            "### Forward read base composition around the 5' end\n"
            + "".join(row(j, c5[j + w]) for j in (-3, -2, -1, 0, 1, 2))
            + "\n\n### Reverse read base composition around the 3' end\n"
            + "".join(row(j, c3[j + w]) for j in (2, 1, 0))
            + "".join(row(j, c3[w - j]) for j in (1, 2, 3)))
    assert text == want == cl.file_text("the genome.fa", "in.bam", w, c5, c3)
    assert text.splitlines()[5] == "-3\t0\t0\t0\t0\t9\t0.00000e+00\t0.00000e+00\t0.00000e+00\t0.00000e+00\t"
    assert f"2\t{2 ** 32 + 5}\t1\t2\t3\t4\t" in text
    pw, p5, p3, f5, f3 = cl.parse_composition_file(text)
    assert pw == w and np.array_equal(p5, c5) and np.array_equal(p3, c3)
    assert f5[2] == cl.fractions(c5[2]) and f3[0] == cl.fractions(c3[0])
    assert host.pss_write_composition(b"f", b"b", str(tmp_path / "no_such_dir" / "o").encode(), w, ptr(c5), ptr(c3)) == 1


def test_rows_end_in_a_tab_like_the_counts_file(host, oracle, tmp_path):
    fwd = np.zeros((3, 16), dtype=np.uint64)
    oracle.write_reports("f", "b", str(tmp_path / "w"), fwd, fwd)
    counts = (tmp_path / "w.pss.counts.txt").read_text()
    c = np.ones((2, 5), dtype=np.uint64)
    ptr = c.ctypes.data_as(C.POINTER(C.c_uint64))
    assert host.pss_write_composition(b"f", b"b", str(tmp_path / "o").encode(), 1, ptr, ptr) == 0
    text = (tmp_path / "o.pss.composition.txt").read_text()
    assert all(ln.endswith("\t") for ln in text.splitlines() if ln and not ln.startswith("#"))
    assert "\n\n\n### Reverse" in text and "\n\n\n### Reverse" in counts       # two blank lines between the blocks in both


# ---- symbols -------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_listed_and_exported(pkg):
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_composition", "pssbam_engine_finish_composition"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert pkg.MAX_COMPOSITION == 30
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^#define PSSBAM_MAX_COMPOSITION 30\b", hdr, re.M)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert re.search(r"^int pssbam_engine_set_composition\(pssbam_engine \*e, int32_t width[^,)]*\);", hdr, re.M)
    assert re.search(r"^int pssbam_engine_finish_composition\(pssbam_engine \*e, uint64_t \*c5, uint64_t \*c3\);$", hdr, re.M)
    assert L.pssbam_engine_set_composition(None, 4) == -1              # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_composition(None, None, None) == -1
    for name in ("set_composition", "finish_composition", "composition"):
        assert hasattr(pkg.Engine, name)
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_composition_width", "pss_composition_fractions", "pss_write_composition"):
        assert hasattr(host, s)


# ---- the command line ------------------------------------------------------------------------------------------------------

def _run_cli(pkg, tmp_path, *args):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"),
                           *args], capture_output=True, text=True, timeout=60)


def _one_line(pr, tmp_path):
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1, pr.stderr
    assert pr.stdout == "" and not list(tmp_path.iterdir())
    return lines[0]


@pytest.mark.parametrize("args", [["-P", ""], ["-P", "0"], ["-P", "31"], ["-P", "-1"], ["-P", "1x"], ["-P", "0x4"]])
def test_cli_refuses_bad_values_before_any_gpu_work(pkg, tmp_path, args):
    line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
    assert "-P" in line and "1..30" in line


EXCLUDED = [(["-G"], "-G"), (["-S", "30,60"], "-S"), (["-C", "map.tsv"], "-C"), (["-H", "100"], "-H"), (["-X", "cpg"], "-X"),
            (["-E", "ds"], "-E"), (["-I"], "-I"), (["-A"], "-A"), (["-n", "3"], "-n"), (["-N", "10"], "-N"), (["-J", "4"], "-J"),
            (["-W", "5"], "-W")]


@pytest.mark.parametrize("other,opt", EXCLUDED, ids=[o for _, o in EXCLUDED])
def test_cli_refuses_the_excluded_options(pkg, tmp_path, other, opt):
    for args in (["-P", "10", *other], [*other, "-P", "10"]):
        line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
        assert "-P" in line and opt in line and "exclude each other" in line


def test_cli_refuses_a_long_region(pkg, tmp_path):
    line = _one_line(_run_cli(pkg, tmp_path, "-P", "5", "-r", "31"), tmp_path)
    assert "-P" in line and "-r <= 30" in line and "-r 31" in line
    pr = _run_cli(pkg, tmp_path, "-P", "30", "-r", "30", "-Q", "20")           # goes with -Q and -r 30: gets as far as the missing input
    assert "Full command" in pr.stderr and pr.stderr.splitlines()[0].endswith(" -Q 20 -P 30")


def test_usage_lists_the_option(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam")], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "-P <w>" in pr.stderr

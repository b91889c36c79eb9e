"""pss-bam -W without a GPU: the margin parser and the writer of the interior file in libpssbam_host.so, the C-ABI symbols of
libpssbam_hip.so, the command line's diagnostics, interior_lib's restatement against the CPU oracle through the row identity,
the golden the unmodified reference wrote for setD, and the conditions under which that golden is not vacuous."""
import ctypes as C
import re
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import interior_lib as il
import mismatch_lib as ml
import pssbam_testlib as tl
import site_context_lib as sc

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
GOLDEN_MARGIN = 15


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


@pytest.fixture(scope="module")
def host(pkg):
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_interior_margin.restype = C.c_int
    L.pss_parse_interior_margin.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.pss_interior_rates.restype = None
    L.pss_interior_rates.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    L.pss_write_interior.restype = C.c_int
    L.pss_write_interior.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.c_uint64]
    return L


def parse(host, arg: bytes):
    """the value, or the diagnostic (str) of a rejection"""
    err = C.create_string_buffer(200)
    v = host.pss_parse_interior_margin(arg, err, len(err))
    if v < 0:
        assert v == -1 and err.value and b"\n" not in err.value, arg
        return err.value.decode()
    return v


# ---- parser ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arg,want", [(b"0", 0), (b"1", 1), (b"15", 15), (b"65535", 65535), (b"007", 7)])
def test_parser_accepts(host, arg, want):
    assert parse(host, arg) == want


@pytest.mark.parametrize("arg", [b"65536", b"-1", b"12x", b"", b"+5", b" 5", b"5 ", b"3.5", b"0x10", b"99999999999999999999"])
def test_parser_rejects_with_a_message(host, arg):
    msg = parse(host, arg)
    assert isinstance(msg, str) and "-W" in msg and "65535" in msg


def test_parser_diagnostics_name_the_problem(host):
    assert "above 65535" in parse(host, b"65536") and "0..65535" in parse(host, b"65536")
    assert "decimal" in parse(host, b"12x") and "needs" in parse(host, b"")


# ---- rates and writer ------------------------------------------------------------------------------------------------

def test_rates_follow_the_rule_of_a_rates_row(host):
    table = (C.c_uint64 * 16)(100, 1, 2, 3, 4, 200, 5, 6, 7, 8, 300, 9, 10, 11, 12, 400)
    rates = (C.c_double * 12)()
    host.pss_interior_rates(table, rates)
    assert ["%.5e" % r for r in rates] == il.expected_rates(list(table))
    assert rates[0] == 1 / (1 + 200 + 8 + 11) and rates[11] == 12 / (2 + 5 + 300 + 12)
    empty_column = (C.c_uint64 * 16)(*[0 if c % 4 == 2 else 5 for c in range(16)])      # no reference G at all: all twelve are zero
    host.pss_interior_rates(empty_column, rates)
    assert list(rates) == [0.0] * 12


def test_write_interior_exact_bytes(host, tmp_path):
    t = [100, 1, 2, 3, 4, 200, 5, 6, 7, 8, 2 ** 32 + 300, 9, 10, 11, 12, 400]
    table = (C.c_uint64 * 16)(*t)
    for q, tail in ((0, ""), (20, ", base quality at least 20 (-Q 20)")):
        prefix = tmp_path / f"out{q}"
        assert host.pss_write_interior(b"the genome.fa", b"in.bam", str(prefix).encode(), 15, q, table, 77) == 0
        want = ("# substitution counts and rates of the read interior: the positions at least 15 bases from both ends of the tallied reads"
                f"{tail}\n"
                "# FASTA: the genome.fa\n"
                "# BAM: in.bam\n"
                "### POS AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT\n"
                "15\t" + "".join(f"{v}\t" for v in t) + "\n"
                "### POS AC AG AT CA CG CT GA GC GT TA TC TG\n"
                "15\t" + "".join(f"{r}\t" for r in il.expected_rates(t)) + "\n"
                "reads\t77\n"
                f"bases\t{sum(t)}\n")
        assert (tmp_path / f"out{q}.pss.interior.txt").read_bytes() == want.encode()
        parsed = il.parse_interior_file(want)
        assert parsed["label"] == 15 and list(parsed["table"]) == t and parsed["reads"] == 77 and parsed["bases"] == sum(t)
    assert host.pss_write_interior(b"f", b"b", str(tmp_path / "no_such_dir" / "o").encode(), 0, 0, table, 1) == 1


def test_rows_are_printed_like_the_counts_and_rates_files(host, oracle, tmp_path):
    """the two rows are those of a counts / rates file whose position-0 row holds the same counts"""
    t = np.array([100, 1, 2, 3, 4, 200, 5, 6, 7, 8, 300, 9, 10, 11, 12, 400], dtype=np.uint64)
    fwd = np.zeros((3, 16), dtype=np.uint64)
    fwd[2] = t
    oracle.write_reports("f", "b", str(tmp_path / "w"), fwd, np.zeros_like(fwd))
    counts_row = next(ln for ln in (tmp_path / "w.pss.counts.txt").read_text().splitlines() if ln.startswith("0\t"))
    rates_row = next(ln for ln in (tmp_path / "w.pss.rates.txt").read_text().splitlines() if ln.startswith("0\t"))
    assert host.pss_write_interior(b"f", b"b", str(tmp_path / "o").encode(), 0, 0, t.ctypes.data_as(C.POINTER(C.c_uint64)), 1) == 0
    lines = (tmp_path / "o.pss.interior.txt").read_text().splitlines()
    assert lines[4] == counts_row and lines[6] == rates_row


# ---- symbols ---------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_listed_and_exported(pkg):
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_interior", "pssbam_engine_finish_interior"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert pkg.MAX_INTERIOR_MARGIN == 65535
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^#define PSSBAM_MAX_INTERIOR_MARGIN 65535\b", hdr, re.M)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert re.search(r"^int pssbam_engine_set_interior\(pssbam_engine \*e, int32_t margin[^,)]*\);", hdr, re.M)
    assert re.search(r"^int pssbam_engine_finish_interior\(pssbam_engine \*e, uint64_t table\[16\], uint64_t \*reads\);$", hdr, re.M)
    assert L.pssbam_engine_set_interior(None, 4) == -1                  # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_interior(None, None, None) == -1
    for name in ("set_interior", "finish_interior", "interior"):
        assert hasattr(pkg.Engine, name)
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_interior_margin", "pss_interior_rates", "pss_write_interior"):
        assert hasattr(host, s)


# ---- the command line ------------------------------------------------------------------------------------------------

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


@pytest.mark.parametrize("args", [["-W", ""], ["-W", "65536"], ["-W", "-1"], ["-W", "1x"], ["-W", "0x4"]])
def test_cli_refuses_bad_values_before_any_gpu_work(pkg, tmp_path, args):
    line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
    assert "-W" in line and "65535" in line


EXCLUDED = [(["-G"], "-G"), (["-S", "30,60"], "-S"), (["-C", "map.tsv"], "-C"), (["-H", "100"], "-H"), (["-X", "cpg"], "-X"),
            (["-E", "ds"], "-E"), (["-I"], "-I"), (["-A"], "-A"), (["-n", "3"], "-n"), (["-N", "10"], "-N"), (["-J", "4"], "-J")]


@pytest.mark.parametrize("other,opt", EXCLUDED, ids=[o for _, o in EXCLUDED])
def test_cli_refuses_the_excluded_options(pkg, tmp_path, other, opt):
    for args in (["-W", "15", *other], [*other, "-W", "15"]):
        line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
        assert "-W" in line and opt in line and "exclude each other" in line


def test_cli_refuses_a_long_region(pkg, tmp_path):
    line = _one_line(_run_cli(pkg, tmp_path, "-W", "5", "-r", "31"), tmp_path)
    assert "-W" in line and "-r <= 30" in line and "-r 31" in line
    pr = _run_cli(pkg, tmp_path, "-W", "5", "-r", "30", "-Q", "20")           # goes with -Q and -r 30: gets as far as the missing input
    assert "Full command" in pr.stderr and pr.stderr.splitlines()[0].endswith(" -Q 20 -W 5")


def test_usage_lists_the_option(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam")], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "-W <d>" in pr.stderr


# ---- the restatement against the CPU oracle ----------------------------------------------------------------------------

def one_length_records(seed: int, x: int, d: int, n: int = 120):
    """unpaired <x>M records of both strands on a contig with lower case, N and IUPAC letters; reads with substitutions,
    N and '=' of their own, one of them inside the interior"""
    rng = np.random.default_rng(seed)
    text = tl.random_contig(rng, 2500)
    recs = []
    for j in range(n):
        s = int(rng.integers(2, len(text) - x - 2))
        subs = {int(p): "ACGTN=R"[int(rng.integers(0, 7))] for p in rng.integers(0, x, size=int(rng.integers(0, 4)))}
        subs[d + int(rng.integers(0, x - 2 * d))] = "ACGTN=R"[int(rng.integers(0, 7))]
        recs.append(il.read_on(text, s, x, subs, name=f"q{j}", flag=16 if rng.integers(0, 2) else 0))
    return [("c", text)], [("c", len(text))], recs


@pytest.mark.parametrize("d", [0, 1, 15])
@pytest.mark.parametrize("which", ["2d+1", "2d+2", "40"])
def test_restatement_equals_the_oracles_rows(oracle, tmp_path, d, which):
    """for unpaired records of one length x: interior(d) == the sum of rows d .. x-d-1 of the oracle's forward table at
    region_len = x - d -- and of its reverse table, which holds the same positions from the other end"""
    x = {"2d+1": 2 * d + 1, "2d+2": 2 * d + 2, "40": 40}[which]
    contigs, refs, recs = one_length_records(100 * d + x, x, d)
    sam = tmp_path / "in.sam"
    tl.write_sam(sam, refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        o = replace(tl.PssOpts(), region_len=x - d, min_read_len=x, max_read_len=x)
        fwd, rev, st = oracle.pss(g, sam, o)
    finally:
        oracle.free_genome(g)
    table, reads, tallied = il.interior(recs, contigs, d, o)
    assert np.array_equal(table, il.rows_sum(fwd, d, x)) and np.array_equal(table, il.rows_sum(rev, d, x))
    assert tallied == int(st[tl.ST_OK]) == reads > 50 and table.sum() > 50 * (x - 2 * d) * 0.8
    assert sum(1 for c in range(16) if c // 4 != c % 4 and table[c]) >= 3
    # the same records with region_len 15 (or x, where shorter): d does not depend on -r
    again = il.interior(recs, contigs, d, replace(tl.PssOpts(), region_len=min(15, x)))
    assert np.array_equal(again[0], table) and again[1:] == (reads, tallied)


def test_restatement_orientation_and_masks():
    text = il.clean_contig(300, seed=5)
    s, L = 50, 40
    p = next(i for i in range(10, 30) if text[s + i] == "C")
    fwd_rec = il.read_on(text, s, L, {p: "T"})                                   # read T on reference C: bin 4 * 3 + 1
    rev_rec = il.read_on(text, s, L, {p: "T"}, flag=16)                          # the same, seen from the other strand: A on G
    for rec, cell in ((fwd_rec, 13), (rev_rec, 2)):
        bins, some = il.record_interior(rec, {"c": text}, 5)
        assert some and bins[cell] == 1 and bins.sum() == 30 and sum(bins[c] for c in (0, 5, 10, 15)) == 29
    low = replace(fwd_rec, qual="I" * p + "#" + "I" * (L - p - 1))               # Phred 2 at the substituted base
    assert il.record_interior(low, {"c": text}, 5, 20)[0][13] == 0 and il.record_interior(low, {"c": text}, 5, 2)[0][13] == 1
    assert il.record_interior(replace(low, qual="*"), {"c": text}, 5, 20)[0][13] == 1      # absent qualities mask nothing
    assert il.record_interior(fwd_rec, {"c": text}, 20)[1] is False and il.record_interior(fwd_rec, {"c": text}, 19)[0].sum() == 2


# ---- the golden ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return il.parse_golden((GOLD / f"interior{GOLDEN_MARGIN}_setD.txt").read_text())


def test_golden_is_not_vacuous(golden):
    assert golden["margin"] == GOLDEN_MARGIN and golden["bases"] == int(golden["table"].sum()) >= 1000
    assert sum(1 for c in range(16) if c // 4 != c % 4 and golden["table"][c]) >= 3
    assert 0 < golden["reads"] < golden["tallied"]


def test_restatement_equals_the_golden(golden):
    """the table the unmodified reference gave through its per-length runs (tests/golden/make_interior_golden.py)"""
    contigs = sc.read_fasta(GOLD / "setD.fa")
    refs, recs = ml.read_sam(GOLD / "setD.sam")
    assert len({il.pss_length(r) for r in recs}) >= 57
    table, reads, tallied = il.interior(recs, contigs, GOLDEN_MARGIN)
    assert np.array_equal(table, golden["table"]) and (reads, tallied) == (golden["reads"], golden["tallied"])
    unpaired, paired = il.split_sam(recs)
    assert unpaired and paired and any(r.flag & 0x80 for r in paired) and any(r.flag & 0x10 for r in recs)

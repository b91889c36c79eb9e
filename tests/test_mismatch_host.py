"""pss-bam -n / -N / -V without a GPU: the two limit parsers and the writer of the mismatches file in libpssbam_host.so,
the C-ABI symbols of libpssbam_hip.so, the command line's diagnostics, the two goldens the unmodified reference wrote for
reduced inputs, and the conditions under which the GPU tests of test_gpu_mismatch.py are not vacuous."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import mismatch_lib as ml
import pssbam_testlib as tl
import site_context_lib as sc

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


@pytest.fixture(scope="module")
def host(pkg):
    L = C.CDLL(str(pkg.LIB_HOST))
    for f in (L.pss_parse_max_mismatches, L.pss_parse_mismatch_hist):
        f.restype = C.c_int
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.pss_write_mismatches.restype = C.c_int
    L.pss_write_mismatches.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def parse(host, which: str, arg: bytes):
    """the value, or the diagnostic (str) of a rejection"""
    err = C.create_string_buffer(200)
    v = (host.pss_parse_max_mismatches if which == "n" else host.pss_parse_mismatch_hist)(arg, err, len(err))
    if v < 0:
        assert v == -1 and err.value and b"\n" not in err.value, arg
        return err.value.decode()
    return v


# ---- parsers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,arg,want", [("n", b"0", 0), ("n", b"1", 1), ("n", b"255", 255), ("n", b"003", 3),
                                            ("N", b"1", 1), ("N", b"255", 255), ("N", b"10", 10), ("N", b"010", 10)])
def test_parsers_accept(host, which, arg, want):
    assert parse(host, which, arg) == want


@pytest.mark.parametrize("which", ["n", "N"])
@pytest.mark.parametrize("arg", [b"256", b"-1", b"12x", b"", b"+5", b" 5", b"5 ", b"3.5", b"0x10", b"99999999999999999999"])
def test_parsers_reject_with_a_message(host, which, arg):
    msg = parse(host, which, arg)
    assert isinstance(msg, str) and f"-{which}" in msg and "255" in msg


def test_parser_diagnostics_name_the_problem(host):
    assert "above 255" in parse(host, "n", b"256") and "0..255" in parse(host, "n", b"256")
    assert "decimal" in parse(host, "n", b"12x") and "decimal" in parse(host, "N", b"0x10")
    assert "at least 1" in parse(host, "N", b"0") and "1..255" in parse(host, "N", b"0")
    assert parse(host, "n", b"0") == 0


# ---- writer ----------------------------------------------------------------------------------------------------------

def test_write_mismatches_exact_bytes(host, tmp_path):
    m = 4
    fwd = (C.c_uint64 * (m + 2))(11, 7, 0, 2 ** 32 + 5, 0, 9)
    rev = (C.c_uint64 * (m + 2))(0, 0, 3, 4, 2 ** 63, 1)
    for tv, word in ((0, "all"), (1, "transversions only")):
        prefix = tmp_path / f"out{tv}"
        assert host.pss_write_mismatches(b"the genome.fa", b"in.bam", str(prefix).encode(), m, tv, fwd, rev) == 0
        want = (f"# mismatches ({word}) of the reads added to the forward / reverse table\n"
                "# FASTA: the genome.fa\n"
                "# BAM: in.bam\n"
                "mismatches\tfwd\trev\n"
                "0\t11\t0\n"
                "1\t7\t0\n"
                "2\t0\t3\n"
                f"3\t{2 ** 32 + 5}\t4\n"
                f"4\t0\t{2 ** 63}\n"
                ">4\t9\t1\n")
        assert (tmp_path / f"out{tv}.pss.mismatches.txt").read_bytes() == want.encode()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out0.pss.mismatches.txt", "out1.pss.mismatches.txt"]


def test_write_mismatches_smallest_limit_and_unwritable_prefix(host, tmp_path):
    fwd, rev = (C.c_uint64 * 3)(1, 2, 3), (C.c_uint64 * 3)(4, 5, 6)
    assert host.pss_write_mismatches(b"f", b"b", str(tmp_path / "o").encode(), 1, 0, fwd, rev) == 0
    assert (tmp_path / "o.pss.mismatches.txt").read_text().splitlines()[3:] == ["mismatches\tfwd\trev", "0\t1\t4", "1\t2\t5", ">1\t3\t6"]
    assert host.pss_write_mismatches(b"f", b"b", str(tmp_path / "no_such_dir" / "o").encode(), 1, 0, fwd, rev) == 1


# ---- symbols ---------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_listed_and_exported(pkg):
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_mismatches", "pssbam_engine_finish_mismatches"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert pkg.MAX_MISMATCHES == 255
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^#define PSSBAM_MAX_MISMATCHES 255\b", hdr, re.M)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert re.search(r"^int pssbam_engine_set_mismatches\(pssbam_engine \*e, int32_t hist_max[^,]*,\s*int32_t max_mismatches[^,]*, int32_t transversions_only\);",
                     hdr, re.M)
    assert re.search(r"^int pssbam_engine_finish_mismatches\(pssbam_engine \*e, uint64_t \*fwd, uint64_t \*rev\);$", hdr, re.M)
    assert L.pssbam_engine_set_mismatches(None, 4, 1, 0) == -1        # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_mismatches(None, None, None) == -1
    for name in ("set_mismatches", "finish_mismatches", "mismatches"):
        assert hasattr(pkg.Engine, name)
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_max_mismatches", "pss_parse_mismatch_hist", "pss_write_mismatches"):
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


@pytest.mark.parametrize("args,opt", [(["-n", ""], "-n"), (["-n", "256"], "-n"), (["-n", "-1"], "-n"), (["-n", "1x"], "-n"),
                                      (["-N", ""], "-N"), (["-N", "0"], "-N"), (["-N", "256"], "-N"), (["-N", "0x4"], "-N"),
                                      (["-n", "1", "-N", "x"], "-N")])
def test_cli_refuses_bad_values_before_any_gpu_work(pkg, tmp_path, args, opt):
    line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
    assert opt in line and "255" in line


def test_cli_V_alone(pkg, tmp_path):
    line = _one_line(_run_cli(pkg, tmp_path, "-V"), tmp_path)
    assert "-V" in line and "-n" in line and "-N" in line


@pytest.mark.parametrize("args", [["-r", "31", "-n", "1"], ["-N", "4", "-r", "31"], ["-r", "100", "-n", "0", "-V"]])
def test_cli_needs_a_one_pass_region_length(pkg, tmp_path, args):
    line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
    assert ("-n" in line or "-N" in line) and "-r" in line and "30" in line


OTHERS = [(["-G"], "-G"), (["-S", "40"], "-S"), (["-C", "no_such_map.tsv"], "-C"), (["-H", "100"], "-H"), (["-X", "cpg"], "-X"),
          (["-E", "ss"], "-E"), (["-I"], "-I"), (["-A"], "-A")]


@pytest.mark.parametrize("mine", [["-n", "1"], ["-N", "4"], ["-N", "4", "-n", "2", "-V"]])
@pytest.mark.parametrize("other,word", OTHERS)
def test_cli_refuses_each_exclusion_pair(pkg, tmp_path, mine, other, word):
    for args in (mine + other, other + mine):
        line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
        assert mine[0] in line and word in line and "exclude each other" in line


def test_cli_usage_names_the_options_and_fragkon_has_none(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-n", "1", "-N", "4", "-V"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr
    for lead in ("-n <k>", "-N <M>", "-V <"):
        assert len([ln for ln in pr.stderr.splitlines() if ln.startswith(lead)]) == 1, lead
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "fragkon"), "-V"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -V." in pr.stderr


# ---- the yardstick ---------------------------------------------------------------------------------------------------

def test_definition_by_hand():
    g = [("c", "ccGATTACAGGnyg")]
    #          01234567890123
    rec = lambda seq, **kw: tl.Rec("r", kw.get("flag", 0), kw.get("rname", "c"), kw.get("pos", 3), 9, kw.get("cigar", [(len(seq), "M")]),  # noqa: E731
                                   tlen=kw.get("tlen", 0), seq=seq, qual="I" * len(seq))
    assert ml.mismatches(rec("GATTACAG"), g) == 0
    assert ml.mismatches(rec("AATTATAG"), g) == 2 and ml.mismatches(rec("AATTATAG"), g, True) == 0       # A/G and T/C: transitions
    assert ml.mismatches(rec("CATTACAT"), g) == 2 and ml.mismatches(rec("CATTACAT"), g, True) == 2       # C/G and T/G: transversions
    assert ml.mismatches(rec("NRTT=CAG"), g) == 0                                                        # N, IUPAC, '=' never count
    assert ml.mismatches(rec("GATTACAGGAAG"), g) == 0 and ml.mismatches(rec("GATTACAGGAAT"), g, True) == 1   # n, y in the reference never count; T/g does
    assert ml.mismatches(rec("gattacat"), g) == 1 and ml.mismatches(rec("TT", pos=1), g) == 2            # case folds on both sides
    assert ml.mismatches(rec("GATTACAG", flag=16), g) == 0 and ml.mismatches(rec("AATTATAG", flag=16), g) == 2   # the strand changes nothing
    assert ml.mismatches(rec("GATTACAG", rname="zz"), g) is None and ml.mismatches(rec("GATTACAG", cigar=[(7, "M")]), g) is None
    assert ml.mismatches(rec("GATTACAG", cigar=[(4, "M"), (4, "M")]), g) is None and ml.mismatches(rec("GATTACAG", cigar=[(8, "=")]), g) is None
    assert ml.mismatches(rec("AATT", flag=1, tlen=-8, cigar=[(8, "M")]), g) == 1                         # l_seq < L: the bases that exist
    assert ml.mismatches(rec("GATTACAG", flag=1, tlen=7), g) is None                                     # a paired read's L is |TLEN|
    assert ml.mismatches(rec("TTTTTTTT", pos=10), g) == 3                                                # on GGnyg and beyond the contig: three T/G inside


def test_definition_by_hand_contig_end():
    g = [("c", "ACGTAC")]
    r = tl.Rec("r", 0, "c", 5, 9, [(4, "M")], seq="CCCC", qual="IIII")       # positions 4, 5 inside (A/C, C/C), 6, 7 outside
    assert ml.mismatches(r, g) == 1
    r0 = tl.Rec("r", 0, "c", 0, 9, [(3, "M")], seq="CCC", qual="III")        # POS 0: s = -1, position -1 outside, then A/C, C/C
    assert ml.mismatches(r0, g) == 1


def test_reduce_and_split_partition_the_input():
    contigs, refs, recs = tl.fuzz_dataset(7301, 3000)
    for tv in (False, True):
        bins = ml.split_by_bin(recs, contigs, 4, tv)
        defined = [r for r in recs if ml.mismatches(r, contigs, tv) is not None]
        assert sum(len(b) for b in bins) == len(defined) and len(bins) == 6
        for k in (0, 1, 3):
            red = ml.reduce_to(recs, contigs, k, tv)
            assert len(recs) - len(red) == sum(len(b) for b in bins[k + 1:])
            assert all(ml.mismatches(r, contigs, tv) is None or ml.mismatches(r, contigs, tv) <= k for r in red)
    text = "".join(tl.sam_line(r) for r in recs)
    assert ml.reduce_sam_text(text, contigs, 1) == "".join(tl.sam_line(r) for r in ml.reduce_to(recs, contigs, 1))


# ---- non-vacuity -----------------------------------------------------------------------------------------------------

def test_fuzz_set_fills_every_bin_and_both_sides_of_every_limit():
    """The set the GPU tests run on.  Among its single-M records on FASTA contigs (2101) every bin 0..4 and the >4 bin hold
    at least 20 records under both modes: 806 / 591 / 349 / 179 / 96 and 80 above, transversions only 1031 / 619 / 271 /
    104 / 47 and 29 above.  At least a tenth of them lies on either side of k = 0 and of k = 1.  Above k = 3 lie 176
    records (8.4 %) and, transversions only, 76 (3.6 %): those very figures rule out a tenth there, so for k = 3 the floor
    is the one of the bins, 20 records on either side, and the counts are pinned."""
    contigs, refs, recs = tl.fuzz_dataset(7301, 3000)
    ctg = dict(contigs)
    for tv, want in ((False, [806, 591, 349, 179, 96, 80]), (True, [1031, 619, 271, 104, 47, 29])):
        ms = [m for m in (ml.span_mismatches(r, ctg, tv) for r in recs) if m is not None]
        counts = np.bincount(np.minimum(ms, 5), minlength=6)
        assert len(ms) == 2101 and counts.tolist() == want
        assert counts.min() >= 20
        for k in (0, 1, 3):
            below, above = int(counts[:k + 1].sum()), int(counts[k + 1:].sum())
            print(f"tv={tv} k={k}: {below} at or below, {above} above, of {len(ms)}")
            if k < 3:
                assert 10 * below >= len(ms) and 10 * above >= len(ms), (tv, k, below, above)
            else:
                assert 10 * below >= len(ms) and above == (76 if tv else 176) and above >= 20
    # and among the records that have an m by the contract (a paired read's L is |TLEN|) likewise
    for tv in (False, True):
        counts = ml.bin_counts(recs, contigs, 4, tv)
        assert counts.min() >= 20
        for k in (0, 1):
            assert 10 * counts[:k + 1].sum() >= counts.sum() and 10 * counts[k + 1:].sum() >= counts.sum()
        assert counts[4:].sum() >= 20


def test_committed_sets_are_cut_by_the_golden_limits():
    ctg = dict(sc.read_fasta(GOLD / "setA.fa"))
    _, recs = ml.read_sam(GOLD / "setA.sam")
    ms = [m for m in (ml.span_mismatches(r, ctg, False, candidates=True) for r in recs) if m is not None]
    assert (sum(m <= 1 for m in ms), sum(m > 1 for m in ms)) == (287, 141)
    ctg = dict(sc.read_fasta(GOLD / "setD.fa"))
    _, recs = ml.read_sam(GOLD / "setD.sam")
    assert len(recs) == 690
    all0, tv0 = ml.reduce_to(recs, ctg, 0, False), ml.reduce_to(recs, ctg, 0, True)
    assert (len(all0), len(tv0)) == (131, 568)
    assert {r.qname for r in all0} < {r.qname for r in tv0}


# ---- goldens ---------------------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


@pytest.mark.parametrize("tag,base,k,tv", [("mism1_setA", "setA", 1, False), ("mismtv0_setD", "setD", 0, True)])
def test_goldens(oracle, tmp_path, tag, base, k, tv):
    """tests/golden/{mism1_setA,mismtv0_setD}.pss.{counts,rates}.txt are what the unmodified reference wrote for the
    reduced inputs (tests/golden/make_mismatch_golden.py); the oracle on the same reduced text reproduces them"""
    contigs = sc.read_fasta(GOLD / f"{base}.fa")
    text = (GOLD / f"{base}.sam").read_text()
    reduced = tmp_path / f"{base}.{tag}.sam"
    reduced.write_text(ml.reduce_sam_text(text, contigs, k, tv))
    assert 100 < len(reduced.read_text().splitlines()) < len(text.splitlines()) - 50
    g = oracle.load_genome(GOLD / f"{base}.fa")
    try:
        fwd, rev, _ = oracle.pss(g, reduced, tl.PssOpts())
        full_f, _, _ = oracle.pss(g, GOLD / f"{base}.sam", tl.PssOpts())
    finally:
        oracle.free_genome(g)
    wf, wr = tl.parse_counts_text((GOLD / f"{tag}.pss.counts.txt").read_text())
    assert np.array_equal(fwd, wf) and np.array_equal(rev, wr)
    assert wf[2:].sum() > 100 and wf.sum() < full_f.sum()
    oracle.write_reports(f"{base}.fa", "x.sam", str(tmp_path / "orc"), fwd, rev)
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"orc.pss.{kind}.txt").read_text()) == report_body((GOLD / f"{tag}.pss.{kind}.txt").read_text()), kind

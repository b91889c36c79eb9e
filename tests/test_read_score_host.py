"""pss-bam -y / -Y without a GPU: the threshold parser, the weight table and the writer of the score file in
libpssbam_host.so, the C-ABI symbols of libpssbam_hip.so, the command line's diagnostics, the two goldens the unmodified
reference wrote for reduced inputs, and the conditions under which the GPU tests of test_gpu_read_score.py are not vacuous."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import mismatch_lib as ml
import pssbam_testlib as tl
import read_score_lib as rs
import site_context_lib as sc

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


@pytest.fixture(scope="module")
def host(pkg):
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_min_score.restype = C.c_int
    L.pss_parse_min_score.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.c_char_p, C.c_size_t]
    L.pss_pmd_weights.restype = None
    L.pss_pmd_weights.argtypes = [C.c_void_p]
    L.pss_write_read_scores.restype = C.c_int
    L.pss_write_read_scores.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def parse(host, arg: bytes):
    """the value, or the diagnostic (str) of a rejection"""
    err, v = C.create_string_buffer(200), C.c_int32(12345)
    rc = host.pss_parse_min_score(arg, C.byref(v), err, len(err))
    if rc:
        assert rc == -1 and err.value and b"\n" not in err.value and v.value == 12345, arg
        return err.value.decode()
    return v.value


# ---- parser ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arg,want", [(b"0", 0), (b"3", 768), (b"-0.5", -128), (b"2.001", 513), (b"-2.001", -512), (b"0.004", 2),
                                      (b"-0.004", -1), (b"0.5", 128), (b"-0", 0), (b"-0.000", 0), (b"003.50", 896), (b"1.0", 256),
                                      (b"7999999.999", 2048000000), (b"-7999999.999", -2047999999)])
def test_parser_accepts(host, arg, want):
    assert parse(host, arg) == want


@pytest.mark.parametrize("arg", [b"", b"+1", b"1.2345", b"1e3", b"-", b" 1", b"1 ", b".5", b"1.", b"--1", b"1.-5", b"0x10", b"1,5",
                                 b"8000000", b"-8000000.0", b"99999999999999999999", b"-.", b"1.2.3"])
def test_parser_rejects_with_a_message(host, arg):
    msg = parse(host, arg)
    assert isinstance(msg, str) and "-y" in msg


# ---- the weight table ------------------------------------------------------------------------------------------------

def test_pmd_weights_follow_the_formula(host):
    w = np.zeros((4, rs.PMD_DIST, rs.PMD_QUAL), dtype=np.int16)
    host.pss_pmd_weights(w.ctypes.data)
    f = rs.pmd_formula()
    assert np.abs(w - f).max() <= 1.5 and np.abs(w.astype(np.int64) - np.rint(f).astype(np.int64)).max() <= 1   # libm may differ in the last place
    assert (w[1, 0] > 0).all() and (w[3, 0] > 0).all() and (w[0, 0] < 0).all() and (w[2, 0] < 0).all()
    assert np.abs(w.astype(np.int64)).max() <= 2047
    assert np.array_equal(w[0], w[2]) and np.array_equal(w[1], w[3])
    # rows d >= 31 equal row 31: the table ends there and the engine freezes larger distances at its last row
    assert w.shape[1] == 32 and rs.PMD_DIST == 32
    committed = rs.committed_pmd_weights()
    assert np.abs(committed - w).max() <= 1
    r = tl.Rec("r", 0, "c", 1, 30, [(80, "M")], seq="C" * 40 + "T" * 40, qual="I" * 80)
    ctg = {"c": "C" * 80}
    wide = np.concatenate([committed, np.repeat(committed[:, 31:32, :], 32, axis=1)], axis=1)              # rows 32..63 = row 31
    assert wide.shape == (4, 64, 64) and rs.score(r, ctg, wide) == rs.score(r, ctg, committed)


# ---- writer ----------------------------------------------------------------------------------------------------------

def test_write_read_scores_exact_bytes(host, tmp_path):
    fwd = (C.c_uint64 * 6)(11, 7, 0, 2 ** 32 + 5, 0, 9)
    rev = (C.c_uint64 * 6)(0, 0, 3, 4, 2 ** 63, 1)
    assert host.pss_write_read_scores(b"the genome.fa", b"in.bam", str(tmp_path / "out").encode(), 3, fwd, rev) == 0
    want = ("# post-mortem-damage score (whole nats, rounded down) of the reads added to the forward / reverse table\n"
            "# FASTA: the genome.fa\n"
            "# BAM: in.bam\n"
            "score\tfwd\trev\n"
            "<-2\t11\t0\n"
            "-2\t7\t0\n"
            "-1\t0\t3\n"
            f"0\t{2 ** 32 + 5}\t4\n"
            f"1\t0\t{2 ** 63}\n"
            ">=2\t9\t1\n")
    assert (tmp_path / "out.pss.pmd.txt").read_bytes() == want.encode()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.pmd.txt"]
    big_f, big_r = (C.c_uint64 * 64)(*range(64)), (C.c_uint64 * 64)(*range(100, 164))
    assert host.pss_write_read_scores(b"f", b"b", str(tmp_path / "o").encode(), 32, big_f, big_r) == 0
    rows = (tmp_path / "o.pss.pmd.txt").read_text().splitlines()[4:]
    assert [r.split("\t")[0] for r in rows] == ["<-31"] + [str(v) for v in range(-31, 31)] + [">=31"] and len(rows) == 64
    assert rows[0] == "<-31\t0\t100" and rows[32] == "0\t32\t132" and rows[63] == ">=31\t63\t163"
    assert host.pss_write_read_scores(b"f", b"b", str(tmp_path / "no_such_dir" / "o").encode(), 32, big_f, big_r) == 1


# ---- symbols ---------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_listed_and_exported(pkg):
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_read_score", "pssbam_engine_finish_read_score"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert (pkg.MAX_SCORE_DIST, pkg.MAX_SCORE_QUAL, pkg.MAX_SCORE_WEIGHT, pkg.MAX_SCORE_HALF) == (64, 64, 2047, 128)
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    for name, v in (("DIST", 64), ("QUAL", 64), ("WEIGHT", 2047), ("HALF", 128)):
        assert re.search(rf"^#define PSSBAM_MAX_SCORE_{name} {v}\b", hdr, re.M), name
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    flat = re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", hdr))          # comments out, one line
    assert ("int pssbam_engine_set_read_score(pssbam_engine *e, const int16_t *weights , int32_t n_dist, int32_t n_qual, int32_t use_filter, "
            "int32_t min_score, int32_t hist_half , int32_t hist_shift );") in flat
    assert re.search(r"^int pssbam_engine_finish_read_score\(pssbam_engine \*e, uint64_t \*fwd, uint64_t \*rev\);$", hdr, re.M)
    w = np.zeros(4, dtype=np.int16)
    assert L.pssbam_engine_set_read_score(None, w.ctypes.data, 1, 1, 0, 0, 0, 0) == -1     # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_read_score(None, None, None) == -1
    for name in ("set_read_score", "finish_read_score", "read_score"):
        assert hasattr(pkg.Engine, name)
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_min_score", "pss_pmd_weights", "pss_write_read_scores"):
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


@pytest.mark.parametrize("arg", ["", "+1", "1.2345", "1e3", "-", "x"])
def test_cli_refuses_bad_values_before_any_gpu_work(pkg, tmp_path, arg):
    assert "-y" in _one_line(_run_cli(pkg, tmp_path, "-y", arg), tmp_path)


@pytest.mark.parametrize("args", [["-r", "31", "-y", "1"], ["-Y", "-r", "31"], ["-r", "100", "-y", "0", "-Y"]])
def test_cli_needs_a_one_pass_region_length(pkg, tmp_path, args):
    line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
    assert ("-y" in line or "-Y" in line) and "-r" in line and "30" in line


OTHERS = [(["-G"], "-G"), (["-S", "40"], "-S"), (["-C", "no_such_map.tsv"], "-C"), (["-H", "100"], "-H"), (["-X", "cpg"], "-X"),
          (["-E", "ss"], "-E"), (["-I"], "-I"), (["-A"], "-A"), (["-n", "1"], "-n"), (["-N", "4"], "-N"), (["-J", "8"], "-J"),
          (["-W", "5"], "-W"), (["-P", "5"], "-P")]


@pytest.mark.parametrize("mine", [["-y", "1"], ["-Y"], ["-Y", "-y", "-2.5"]])
@pytest.mark.parametrize("other,word", OTHERS)
def test_cli_refuses_each_exclusion_pair(pkg, tmp_path, mine, other, word):
    for args in (mine + other, other + mine):
        line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
        assert mine[0] in line and word in line and "exclude each other" in line


def test_cli_usage_names_the_options_and_fragkon_has_none(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-y", "1", "-Y"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr
    for lead in ("-y <t>", "-Y <"):
        assert len([ln for ln in pr.stderr.splitlines() if ln.startswith(lead)]) == 1, lead
    assert "1/256 nat" in pr.stderr and "no parity" in pr.stderr
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "fragkon"), "-Y"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -Y." in pr.stderr


# ---- the yardstick ---------------------------------------------------------------------------------------------------

def test_definition_by_hand():
    g = {"c": "ttCCGGAnCG"}
    #           0123456789
    W = np.arange(4 * 3 * 2).reshape(4, 3, 2) + 100          # W[kind][d][q] = 100 + 6 kind + 2 d + q
    rec = lambda seq, qual=None, **kw: tl.Rec("r", kw.get("flag", 0), kw.get("rname", "c"), kw.get("pos", 3), 9,  # noqa: E731
                                              kw.get("cigar", [(len(seq), "M")]), tlen=kw.get("tlen", 0), seq=seq,
                                              qual=qual if qual is not None else "!" * len(seq))
    w = lambda kind, d, q: 100 + 6 * kind + 2 * d + q         # noqa: E731
    # CCGGA read as itself: C at i = 0, 1 (kind 0, d = 0, 1), G at i = 2, 3 (kind 2, d = L-1-i = 2, 1); A/A adds nothing
    assert rs.score(rec("CCGGA"), g, W) == w(0, 0, 0) + w(0, 1, 0) + w(2, 2, 0) + w(2, 1, 0)
    # C->T at i = 1, G->A at i = 2; quality 1 and above land in the last column
    assert rs.score(rec("CTAGA", "!\"#$%"), g, W) == w(0, 0, 0) + w(1, 1, 1) + w(3, 2, 1) + w(2, 1, 1)
    # the reverse strand swaps the kinds, not the distances
    assert rs.score(rec("CTAGA", flag=16), g, W) == w(2, 0, 0) + w(3, 1, 0) + w(1, 2, 0) + w(0, 1, 0)
    # distances saturate at the last row: L = 8 over CCGGAnCG, G at i = 2 has L-1-i = 5 -> row 2; n and N never count
    assert rs.score(rec("CCGGANCG"), g, W) == w(0, 0, 0) + w(0, 1, 0) + w(2, 2, 0) + w(2, 2, 0) + w(0, 2, 0) + w(2, 0, 0)
    # other pairs (C under A, G under T, T under C) add nothing; absent qualities land in the last column
    assert rs.score(rec("AATTA"), g, W) == 0 and rs.score(rec("CCGGA", "*"), g, W) == w(0, 0, 1) + w(0, 1, 1) + w(2, 2, 1) + w(2, 1, 1)
    # a minimum base quality takes positions out; 0xFF is never below
    assert rs.score(rec("CCGGA", "5!5!5"), g, W, min_bq=20) == w(0, 0, 1) + w(2, 2, 1) and rs.score(rec("CCGGA", "*"), g, W, min_bq=93) > 0
    # not defined: unknown contig, CIGAR other than <L>M, a paired read whose |TLEN| is not the CIGAR length
    assert rs.score(rec("CCGGA", rname="zz"), g, W) is None and rs.score(rec("CCGGA", cigar=[(4, "M")]), g, W) is None
    assert rs.score(rec("CCGGA", flag=1, tlen=4), g, W) is None
    # l_seq < L: the bases that exist, distances by L; beyond the contig end nothing counts
    assert rs.score(rec("CC", flag=1, tlen=-5, cigar=[(5, "M")]), g, W) == w(0, 0, 0) + w(0, 1, 0)
    assert rs.score(rec("CGCG", pos=9), g, W) == w(0, 0, 0) + w(2, 2, 0)
    assert rs.score_bin(-1, 2, 8) == 1 and rs.score_bin(-257, 2, 8) == 0 and rs.score_bin(-100000, 2, 8) == 0 and rs.score_bin(255, 2, 8) == 2
    assert rs.score_bin(256, 2, 8) == 3 and rs.score_bin(10 ** 6, 2, 8) == 3 and rs.score_bin(-3, 128, 0) == 125


def test_reduce_and_split_partition_the_input():
    contigs, refs, recs = tl.fuzz_dataset(*rs.FUZZ)
    W = rs.committed_pmd_weights()
    bins = rs.split_by_bin(recs, contigs, W, 32, 8)
    defined = [r for r in recs if rs.score(r, contigs, W) is not None]
    assert sum(len(b) for b in bins) == len(defined) and len(bins) == 64
    for t in (-2, 0, 1):
        red = rs.reduce_to(recs, contigs, W, 256 * t)
        assert len(recs) - len(red) == sum(len(b) for b in bins[:32 + t])
    text = "".join(tl.sam_line(r) for r in recs)
    assert rs.reduce_sam_text(text, contigs, W, 0) == "".join(tl.sam_line(r) for r in rs.reduce_to(recs, contigs, W, 0))


# ---- non-vacuity -----------------------------------------------------------------------------------------------------

def test_fuzz_set_has_reads_on_both_sides_of_every_threshold():
    contigs, refs, recs = tl.fuzz_dataset(*rs.FUZZ)
    ctg, tabs = dict(contigs), rs.tables()
    assert 200 <= len(recs) <= 1000
    for name, q, t in rs.CUTS:
        S = np.array([s for s in (rs.score(r, ctg, tabs[name], q) for r in recs) if s is not None])
        kept = int((S >= t).sum())
        print(f"{name} min_bq={q} min_score={t}: keeps {kept} of {len(S)}")
        assert len(S) == 626 and 0.2 * len(S) <= kept <= 0.8 * len(S), (name, q, t, kept, len(S))
        assert (S < 0).sum() >= 20 and (S > 0).sum() >= 20


def test_every_histogram_shape_fills_its_bins():
    """per shape and flag class: the four-bin shapes have every bin filled by at least one class, the 256-bin shapes both
    clamp bins and a spread of bins between them, and negative scores are there to be floored"""
    from test_gpu_length_hist import split_by_flag
    contigs, refs, recs = tl.fuzz_dataset(*rs.FUZZ)
    tabs = rs.tables()
    for name, half, shift in rs.HIST_SHAPES:
        used = np.zeros(2 * half, dtype=bool)
        for part in split_by_flag(recs).values():
            used |= np.array([len(b) > 0 for b in rs.split_by_bin(part, contigs, tabs[name], half, shift)])
        print(f"{name} half={half} shift={shift}: {int(used.sum())} of {2 * half} bins used")
        if half == 2:
            assert used.all(), (name, half, shift)
        elif shift == 0:
            assert used[0] and used[-1] and used.sum() >= 64, (name, half, shift, int(used.sum()))
        else:
            assert used[-1] and used[:half].sum() >= 20 and used[half:].sum() >= 20, (name, half, shift, int(used.sum()))


def test_committed_sets_are_cut_by_the_golden_thresholds():
    W = rs.committed_pmd_weights()
    for base, t, want in (("setD", 3, (388, 690)), ("setA", 0, (64, 441))):
        ctg = dict(sc.read_fasta(GOLD / f"{base}.fa"))
        _, recs = ml.read_sam(GOLD / f"{base}.sam")
        S = [s for s in (rs.score(r, ctg, W) for r in recs) if s is not None]
        assert (sum(s >= 256 * t for s in S), len(S)) == want


# ---- goldens ---------------------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


@pytest.mark.parametrize("tag,base,t", [("pmd3_setD", "setD", 3), ("pmd0_setA", "setA", 0)])
def test_goldens(oracle, tmp_path, tag, base, t):
    """tests/golden/{pmd3_setD,pmd0_setA}.pss.{counts,rates}.txt are what the unmodified reference wrote for the reduced
    inputs (tests/golden/make_read_score_golden.py); the oracle on the same reduced text reproduces them"""
    contigs = sc.read_fasta(GOLD / f"{base}.fa")
    text = (GOLD / f"{base}.sam").read_text()
    reduced = tmp_path / f"{base}.{tag}.sam"
    reduced.write_text(rs.reduce_sam_text(text, contigs, rs.committed_pmd_weights(), 256 * t))
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

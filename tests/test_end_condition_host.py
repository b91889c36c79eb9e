"""pss-bam -E without a GPU: the C ABI carries the setter pair, the command line parses the option and refuses bad uses
of it before any work, the report writer writes the three files, and the yardstick the GPU tests use -- the CPU oracle
on the input reduced to the marked unpaired records -- is itself checked against a direct count and reproduces files
the unmodified reference wrote for the damaged fixture setD."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import end_condition_lib as ec
import pssbam_testlib as tl
import site_context_lib as sc

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
CASES = {"ss": (1, 13, 13, 0), "ds": (1, 13, 2, 0), "ss3": (3, 13, 13, 0), "ss_q20": (1, 13, 13, 20)}


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_pkg()


def test_setter_pair_is_declared_listed_and_exported(pkg):
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^#define PSSBAM_MAX_END_DEPTH 8\b", hdr, re.M)
    assert re.search(r"^int pssbam_engine_set_end_condition\(pssbam_engine \*e, int32_t depth, int32_t cell5, int32_t cell3\);$", hdr, re.M)
    assert re.search(r"^int pssbam_engine_finish_end_condition\(pssbam_engine \*e, unsigned long \*fwd_c, unsigned long \*rev_c, uint64_t reads\[4\]\);$",
                     hdr, re.M)
    assert pkg.MAX_END_DEPTH == 8 and pkg.END_PRESETS == ec.PRESETS == {"ss": (13, 13), "ds": (13, 2)}
    L = pkg.hip_lib()
    L.pssbam_last_error.restype = C.c_char_p
    for s in ("pssbam_engine_set_end_condition", "pssbam_engine_finish_end_condition"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert L.pssbam_engine_set_end_condition(None, 1, 13, 13) == -1        # PSSBAM_EINVAL, not a dereference
    assert L.pssbam_engine_finish_end_condition(None, None, None, None) == -1
    assert L.pssbam_last_error()
    for name in ("set_end_condition", "finish_end_condition", "end_condition"):
        assert hasattr(pkg.Engine, name)


def test_cells_are_the_columns_of_the_counts_file():
    cols = (GOLD / "cond_ss_setD.pss.counts.txt").read_text().split("### POS ")[1].splitlines()[0].split()
    assert cols[13] == "TC" and cols[2] == "AG" and ec.cell_of("T", "C") == 13 and ec.cell_of("A", "G") == 2 and ec.cell_of("N", "C") is None


# ---- option parsing (the front end's parser, in libpssbam_host.so) and refusals -------------------------------------

def parse(pkg, arg: str):
    H = C.CDLL(str(pkg.PKG_DIR / "libpssbam_host.so"))
    d, c5, c3 = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    err = C.create_string_buffer(300)
    rc = H.pss_parse_end_condition(arg.encode(), C.byref(d), C.byref(c5), C.byref(c3), err, C.c_size_t(300))
    return (d.value, c5.value, c3.value) if rc == 0 else err.value.decode()


def test_option_parsing(pkg):
    assert parse(pkg, "ss") == (1, 13, 13) and parse(pkg, "ds") == (1, 13, 2)
    assert parse(pkg, "ss,3") == (3, 13, 13) and parse(pkg, "ds,8") == (8, 13, 2) and parse(pkg, "ss,1") == (1, 13, 13)
    for bad in ("", "s", "xs", "SS", "ss,", "ss,0", "ss,9", "ss,-1", "ss,2x", "ss3", "ss, 3", "ds,1,2", "ss,+2"):
        msg = parse(pkg, bad)
        assert isinstance(msg, str) and msg.startswith("-E ") and "\n" not in msg, (bad, msg)


REFUSED = [(["-E", "sx"], "preset"), (["-E", "ss,9"], "depth"), (["-E", ""], "preset"),
           (["-E", "ss", "-G"], "-G"), (["-G", "-E", "ds"], "-G"), (["-E", "ss", "-S", "40"], "-S"), (["-E", "ss", "-C", "no.map"], "-C"),
           (["-E", "ds,2", "-H", "100"], "-H"), (["-X", "cpg", "-E", "ss"], "-X"), (["-E", "ss", "-r", "31"], "30"),
           (["-r", "100", "-E", "ds"], "30"), (["-E", "ss,3", "-r", "2"], "depth")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_cli_refuses_before_any_work(pkg, args, word, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(tmp_path / "no.fa"), "-B", str(tmp_path / "no.bam"), "-o", str(tmp_path / "out"), *args],
                        capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    lines = pr.stderr.splitlines()
    assert len(lines) == 1 and "-E" in lines[0] and word in lines[0], pr.stderr
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr
    assert pr.stdout == "" and list(tmp_path.iterdir()) == []


def test_cli_usage_names_the_option_and_fragkon_has_none(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-E", "ss"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr
    assert len([ln for ln in pr.stderr.splitlines() if ln.startswith("-E <ss|ds>[,<d>]")]) == 1
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "fragkon"), "-E", "ss"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -E." in pr.stderr


# ---- the report writer -------------------------------------------------------------------------------------------------

def test_report_writer_writes_the_three_files(pkg, oracle, tmp_path):
    H = C.CDLL(str(pkg.PKG_DIR / "libpssbam_host.so"))
    rng = np.random.default_rng(3)
    fwd = rng.integers(0, 1000, size=(17, 16)).astype(np.uint64)
    rev = rng.integers(0, 1000, size=(17, 16)).astype(np.uint64)
    prefix = tmp_path / "rep"
    rc = H.pss_write_labelled(b"g.fa", b"in.bam", str(prefix).encode(), b"cond", 15, fwd.ctypes.data_as(C.c_void_p), rev.ctypes.data_as(C.c_void_p))
    reads = (C.c_uint64 * 4)(549, 120, 106, 2 ** 40)
    assert rc == 0 and H.pss_write_end_reads(str(prefix).encode(), reads) == 0
    assert sorted(p.name for p in tmp_path.iterdir()) == ["rep.cond.pss.counts.txt", "rep.cond.pss.rates.txt", "rep.cond.pss.reads.txt"]
    assert (tmp_path / "rep.cond.pss.reads.txt").read_text() == f"unpaired_reads\t549\nmarked_5p\t120\nmarked_3p\t106\nmarked_both\t{2 ** 40}\n"
    counts = (tmp_path / "rep.cond.pss.counts.txt").read_text()
    gf, gr = tl.parse_counts_text(counts)
    assert np.array_equal(gf, fwd) and np.array_equal(gr, rev)
    assert f"### OUT: {prefix}.cond.pss.counts.txt" in counts.splitlines()
    oracle.write_reports("g.fa", "in.bam", str(tmp_path / "orc"), fwd, rev)       # the unchanged table format
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"rep.cond.pss.{kind}.txt").read_text()) == report_body((tmp_path / f"orc.pss.{kind}.txt").read_text())
    assert H.pss_write_end_reads(str(tmp_path / "no_such_dir" / "x").encode(), reads) == 1


def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


# ---- the yardstick ---------------------------------------------------------------------------------------------------

def test_marks_by_hand():
    g = [("c", "ccGATTACAGGg")]
    #          012345678901
    r = tl.Rec("r", 0, "c", 3, 9, [(8, "M")], seq="AATTATAG", qual="IIIIII!I")      # on GATTACAG: A/G at 0, T/C at 5
    assert ec.marks(g, r, 1, 2, 15) == (True, False) and ec.marks(g, r, 1, 2, 10) == (True, True)      # AG at the 5' end, GG at the 3' end
    assert ec.marks(g, r, 2, 13, 13) == (False, False) and ec.marks(g, r, 3, 13, 13) == (False, True) and ec.marks(g, r, 6, 13, 13) == (True, True)
    assert ec.marks(g, r, 3, 13, 13, min_bq=20) == (False, True) and ec.marks(g, r, 2, 12, 12, min_bq=20) == (False, False)
    rv = tl.Rec("v", 16, "c", 3, 9, [(8, "M")], seq="AATTATAG", qual="IIIIII!I")    # read orientation: CTATAATT on CTGTAATC
    assert ec.marks(g, rv, 1, 5, 13) == (True, True) and ec.marks(g, rv, 3, 2, 5) == (True, False) and ec.marks(g, rv, 2, 2, 15) == (False, True)
    assert ec.marks(g, rv, 2, 15, 15, min_bq=20) == (False, True)                     # the masked base is o[1] now
    for other in (tl.Rec("p", 1, "c", 3, 9, [(8, "M")], seq="AATTATAG", qual="I" * 8), tl.Rec("s", 0, "c", 3, 9, [], seq="*", qual="*"),
                  tl.Rec("m", 0, "zz", 3, 9, [(8, "M")], seq="AATTATAG", qual="I" * 8), tl.Rec("e", 0, "c", 8, 9, [(8, "M")], seq="AATTATAG", qual="I" * 8)):
        assert ec.marks(g, other, 1, 2, 10) == (False, False)
    text = "@SQ\tSN:c\tLN:12\n" + tl.sam_line(r) + tl.sam_line(rv) + "p\t1\tc\t3\t9\t8M\t*\t0\t8\tAATTATAG\tIIIIIIII\n"
    assert ec.reduce_sam_text(text, g, 1, 2, 15, "5") == "@SQ\tSN:c\tLN:12\n" + tl.sam_line(r)
    assert ec.reduce_sam_text(text, g, 1, 5, 13, "both") == "@SQ\tSN:c\tLN:12\n" + tl.sam_line(rv)
    assert ec.reduce_sam_text(text, g, 1, 5, 13, "unpaired").count("\n") == 3
    assert [x.qname for x in ec.reduce_recs(g, [r, rv], 1, 2, 13, "3")] == ["v"]


@pytest.fixture(scope="module")
def fuzz(oracle):
    contigs, refs, recs = tl.fuzz_dataset(8101, 2000)
    recs = ec.plant_damage(contigs, recs, np.random.default_rng(8102), 0.5)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    yield contigs, refs, recs, g
    oracle.free_genome(g)


OPTS = [(tl.PssOpts(region_len=15), (1, 13, 13)), (tl.PssOpts(region_len=15), (1, 13, 2)), (tl.PssOpts(region_len=30, min_mq=10, up_ctx="CT"), (3, 13, 2)),
        (tl.PssOpts(region_len=1, max_read_len=60), (1, 0, 15)), (tl.PssOpts(region_len=8, down_ctx="AG", merged_only=True), (8, 5, 10))]


@pytest.mark.parametrize("o,cond", OPTS)
def test_oracle_on_reduced_input_equals_direct_count(oracle, fuzz, tmp_path, o, cond):
    """the yardstick: reducing the input to the marked unpaired records == adding their contribution a second time"""
    contigs, refs, recs, g = fuzz
    want = ec.expected(oracle, g, tmp_path, refs, contigs, recs, o, *cond)
    direct = ec.direct_counts(contigs, recs, o, *cond)
    for k in range(3):
        assert np.array_equal(want[k], direct[k]), (k, o, cond)
    assert want[2][1] >= 10 and want[2][2] >= 10 and want[2][0] >= want[2][1] >= want[2][3]
    assert int(want[0][0].sum()) == want[2][2] or "N" in "".join(s for _, s in contigs).upper()     # one context add per record


# ---- goldens ---------------------------------------------------------------------------------------------------------

def golden_reads(case: str) -> list:
    lines = (GOLD / f"cond_{case}_setD.pss.reads.txt").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in lines] == ["unpaired_reads", "marked_5p", "marked_3p", "marked_both"]
    return [int(ln.split("\t")[1]) for ln in lines]


def test_fixture_is_not_vacuous():
    """at d = 1 either preset marks at least 20 reads at the 5' end, at the 3' end and at both (the reference's counts)"""
    for case in ("ss", "ds"):
        reads = golden_reads(case)
        assert min(reads[1:]) >= 20 and reads[0] > reads[1] and reads[0] > reads[2], (case, reads)
    recs = [ln.split("\t") for ln in (GOLD / "setD.sam").read_text().splitlines() if not ln.startswith("@")]
    assert 500 <= len(recs) <= 700 and all(15 <= len(f[9]) <= 80 for f in recs)
    paired = sum(int(f[1]) & 1 for f in recs)
    assert 0.12 * len(recs) < paired < 0.28 * len(recs) and 0.3 * len(recs) < sum(bool(int(f[1]) & 16) for f in recs) < 0.7 * len(recs)
    assert sum(min(ord(c) - 33 for c in f[10][:3] + f[10][-3:]) < 20 for f in recs) >= 20


@pytest.mark.parametrize("case", list(CASES))
def test_goldens(oracle, tmp_path, case):
    """tests/golden/cond_<case>_setD.pss.* are what the unmodified reference wrote for setD.sam reduced to the marked
    unpaired records (tests/golden/make_end_condition_golden.py); the oracle on the same reduced text reproduces them,
    and so does the reference itself where it is built"""
    d, c5, c3, q = CASES[case]
    contigs = sc.read_fasta(GOLD / "setD.fa")
    text = (GOLD / "setD.sam").read_text()
    g = oracle.load_genome(GOLD / "setD.fa")
    got, reads = {}, []
    try:
        for which in ("unpaired", "5", "3", "both"):
            red = ec.reduce_sam_text(text, contigs, d, c5, c3, which, q)
            sam = tmp_path / f"setD.{which}.sam"
            sam.write_text(bq.mask_sam_text(red, q) if q else red)
            got[which] = oracle.pss(g, sam, tl.PssOpts())
            reads.append(int(got[which][2][tl.ST_OK]))
            if tl.have_ref():
                rf, rr, _, _, _ = tl.run_ref_pss(GOLD / "setD.fa", sam, tmp_path / f"ref_{which}", tl.PssOpts())
                assert np.array_equal(rf, got[which][0]) and np.array_equal(rr, got[which][1]), which
    finally:
        oracle.free_genome(g)
    fwd, rev = got["3"][0], got["5"][1]
    wf, wr = tl.parse_counts_text((GOLD / f"cond_{case}_setD.pss.counts.txt").read_text())
    assert np.array_equal(fwd, wf) and np.array_equal(rev, wr) and reads == golden_reads(case)
    assert wf[2:].sum() > 500 and wr[2:].sum() > 500
    oracle.write_reports("setD.fa", "x.sam", str(tmp_path / "orc"), fwd, rev)
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"orc.pss.{kind}.txt").read_text()) == report_body((GOLD / f"cond_{case}_setD.pss.{kind}.txt").read_text()), kind

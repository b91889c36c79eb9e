"""pss-bam -X cpg without a GPU: the C ABI carries the setter pair, the command line refuses bad uses of the option
before any work, and the yardstick the GPU tests use -- the CPU oracle on a copy of the input with the read bases at
the other kind of site set to N -- is itself checked against a direct count that skips those positions, and
reproduces tables the unmodified reference wrote."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl
import site_context_lib as sc

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"
SEED = 9401


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_pkg()


def test_setter_pair_is_declared_listed_and_exported(pkg):
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^#define PSSBAM_SITE_NONE 0\b", hdr, re.M) and re.search(r"^#define PSSBAM_SITE_CPG 1\b", hdr, re.M)
    assert re.search(r"^int pssbam_engine_set_site_context\(pssbam_engine \*e, int32_t mode\);$", hdr, re.M)
    assert re.search(r"^int pssbam_engine_finish_site_context\(pssbam_engine \*e, unsigned long \*fwd_in, unsigned long \*rev_in\);$", hdr, re.M)
    assert (pkg.SITE_NONE, pkg.SITE_CPG) == (0, 1)
    L = pkg.hip_lib()
    L.pssbam_last_error.restype = C.c_char_p
    for s in ("pssbam_engine_set_site_context", "pssbam_engine_finish_site_context"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert L.pssbam_engine_set_site_context(None, 1) == -1            # PSSBAM_EINVAL, not a dereference
    assert L.pssbam_engine_finish_site_context(None, None, None) == -1
    assert L.pssbam_last_error()
    for name in ("set_site_context", "finish_site_context", "site_context"):
        assert hasattr(pkg.Engine, name)


REFUSED = [(["-X", "cpgx"], "-X"), (["-X", ""], "-X"), (["-X", "CpG"], "-X"), (["-X", "chh"], "-X"),
           (["-X", "cpg", "-G"], "-G"), (["-G", "-X", "cpg"], "-G"), (["-X", "cpg", "-S", "40"], "-S"),
           (["-X", "cpg", "-C", "no.map"], "-C"), (["-X", "cpg", "-H", "100"], "-H"), (["-H", "100", "-X", "cpg"], "-H")]


@pytest.mark.parametrize("args,other", REFUSED)
def test_cli_refuses_before_any_work(pkg, args, other, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(tmp_path / "no.fa"), "-B", str(tmp_path / "no.bam"), "-o", str(tmp_path / "out"), *args],
                        capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    lines = pr.stderr.splitlines()
    assert len(lines) == 1 and "-X" in lines[0] and other in lines[0], pr.stderr
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr
    assert pr.stdout == "" and list(tmp_path.iterdir()) == []


def test_cli_X_alone_prints_the_reference_usage(pkg):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-X", "cpg"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1
    assert pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr and "-X" not in pr.stderr


def test_fragkon_has_no_X(pkg):
    exe = pkg.PKG_DIR / "bin" / "fragkon"
    pr = subprocess.run([str(exe), "-X", "cpg"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -X." in pr.stderr


def test_in_cpg_and_the_masker():
    g = "ACGTCCGGCATG"
    #    012345678901
    assert [p for p in range(-1, len(g) + 1) if sc.in_cpg(g, p)] == [1, 2, 5, 6]
    assert list(np.flatnonzero(sc.cpg_flags(g.lower()))) == [1, 2, 5, 6]
    assert not sc.in_cpg("CG"[:1], 0) and not sc.in_cpg("G", 0) and sc.in_cpg("CG", 0) and sc.in_cpg("CG", 1)
    f = sc.cpg_flags(g)
    assert sc.mask_seq("ACGTCC", f, 0, True) == "NCGNNC" and sc.mask_seq("ACGTCC", f, 0, False) == "ANNTCN"
    assert sc.mask_seq("TTTT", f, 10, False) == "TTNN" and sc.mask_seq("TTTT", f, -2, False) == "NNTN"   # outside the contig
    assert sc.mask_seq("*", f, 3, True) == "*"
    text = "@SQ\tSN:c\tLN:12\nr\t0\tc\t2\t9\t3M\t*\t0\t0\tAAA\t!I!\tRG:Z:x\nq\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\nz\t0\tother\t1\t9\t2M\t*\t0\t0\tCG\tII\n"
    assert sc.mask_sam_text(text, [("c", g.lower())], True) == text.replace("AAA", "AAN")
    assert sc.mask_sam_text(text, [("c", g)], False) == text.replace("AAA", "NNA")
    recs = [tl.Rec("r", 0, "c", 2, 9, [(3, "M")], seq="AAA", qual="!I!"), tl.Rec("z", 0, "other", 1, 9, [(2, "M")], seq="CG", qual="II")]
    assert [r.seq for r in sc.mask_recs([("c", g)], recs, True)] == ["AAN", "CG"]


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(SEED, 3000)
    d = tmp_path_factory.mktemp("site")
    sams = {None: d / "plain.sam", True: d / "in.sam", False: d / "out.sam"}
    tl.write_sam(sams[None], refs, recs)
    for keep in (True, False):
        tl.write_sam(sams[keep], refs, sc.mask_recs(contigs, recs, keep))
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    yield contigs, refs, recs, sams, g
    oracle.free_genome(g)


OPTS = [tl.PssOpts(region_len=15), tl.PssOpts(region_len=31, min_mq=10, up_ctx="CT", down_ctx="ACGTN"), tl.PssOpts(region_len=62)]


@pytest.mark.parametrize("keep_in", [True, False])
def test_oracle_on_masked_sam_equals_direct_count(oracle, fuzz, keep_in):
    """the yardstick: N-masking the SAM == leaving the positions out of the count"""
    contigs, refs, recs, sams, g = fuzz
    for o in OPTS:
        pf, pr_, pst = oracle.pss(g, sams[None], o)
        mf, mr, mst = oracle.pss(g, sams[keep_in], o)
        df, dr = sc.direct_counts(contigs, recs, o, keep_in)
        assert np.array_equal(mf, df) and np.array_equal(mr, dr), o
        zf, zr = sc.direct_counts(contigs, recs, o, None)
        assert np.array_equal(pf, zf) and np.array_equal(pr_, zr), o          # (the direct count itself, unmasked)
        assert np.array_equal(pst, mst)                                       # no record changes its status
        assert np.array_equal(pf[:2], mf[:2]) and np.array_equal(pr_[:2], mr[:2])   # context rows: reference only


def test_fixture_is_rich_in_both_kinds(oracle, fuzz):
    """IN and OUT are both well populated and partition the plain tables: a fixture too poor in CpG fails here, not on
    the GPU"""
    contigs, refs, recs, sams, g = fuzz
    for o in OPTS:
        pf, pr_, _ = oracle.pss(g, sams[None], o)
        inf, inr, _ = oracle.pss(g, sams[True], o)
        of, orv, _ = oracle.pss(g, sams[False], o)
        for t_in, t_out, t in ((inf, of, pf), (inr, orv, pr_)):
            assert t_in[2:].sum() > 500 and t_out[2:].sum() > 500, o
            assert np.array_equal(t_in[2:] + t_out[2:], t[2:]), o
            assert not t_in[2:, [0, 3, 4, 7, 8, 11, 12, 15]].any()            # an in-context cell has reference base C or G


def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


@pytest.mark.parametrize("tag,keep_in", [("cpg", True), ("noncpg", False)])
def test_goldens(oracle, tmp_path, tag, keep_in):
    """tests/golden/{cpg,noncpg}_setA.pss.{counts,rates}.txt are what the unmodified reference wrote for setA.sam
    masked both ways (tests/golden/make_site_context_golden.py); the oracle on the same masked text reproduces them"""
    contigs = sc.read_fasta(GOLD / "setA.fa")
    masked = tmp_path / f"setA.{tag}.sam"
    masked.write_text(sc.mask_sam_text((GOLD / "setA.sam").read_text(), contigs, keep_in))
    g = oracle.load_genome(GOLD / "setA.fa")
    try:
        fwd, rev, _ = oracle.pss(g, masked, tl.PssOpts())
    finally:
        oracle.free_genome(g)
    want_c = (GOLD / f"{tag}_setA.pss.counts.txt").read_text()
    wf, wr = tl.parse_counts_text(want_c)
    assert np.array_equal(fwd, wf) and np.array_equal(rev, wr)
    assert wf[2:].sum() > 100
    oracle.write_reports("setA.fa", "x.sam", str(tmp_path / "orc"), fwd, rev)
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"orc.pss.{kind}.txt").read_text()) == report_body((GOLD / f"{tag}_setA.pss.{kind}.txt").read_text()), kind

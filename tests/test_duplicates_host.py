"""Duplicate flagging (pss-bam -d, fragkon -d) without a GPU: the Python restatement of the definition (duplicates_lib) against the
CPU oracle and the unmodified reference, the report writer of libpssbam_host.so against the committed golden file, the C-ABI
symbols, and the command lines' refusals."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import duplicates_lib as dl
import pssbam_testlib as tl

# every base letter a fuzz contig holds is in both context sets: the oracle then tallies exactly the candidates
ALL_CTX = "ACGTNRYMKSWBDHV"
SEEDS = [5101, 5102]


def fuzz(seed, n=500, with_rg=False):
    contigs, refs, recs = tl.fuzz_dataset(seed, n, with_rg=with_rg)
    return contigs, refs, dl.with_copies(recs, seed, max_copies=2)


def setup_of(contigs, refs, **kw):
    return dl.Setup(refs, {n: len(s) for n, s in contigs}, **kw)


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_write_duplicates.restype = C.c_int
    L.pss_write_duplicates.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int]
    return L


# ---- the model against the oracle ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_eligibility_is_the_oracles_candidate_test_record_by_record(oracle, tmp_path, seed):
    """each unpaired record alone: the oracle tallies it iff the model calls it eligible (with every base in -U / -D a candidate is
    tallied), and with FLAG 0x400 set it moves from OK to FILTERED -- which is what the engine's flagging relies on"""
    contigs, refs, recs = fuzz(seed)
    o = tl.PssOpts(region_len=4, min_mq=20, min_read_len=10, max_read_len=120, up_ctx=ALL_CTX, down_ctx=ALL_CTX)
    s = setup_of(contigs, refs, pss=o)
    v = dl.judge_recs(recs, s)
    fa, sam = tmp_path / "g.fa", tmp_path / "one.sam"
    tl.write_fasta(fa, contigs)
    g = oracle.load_genome(fa)
    try:
        seen = set()
        for r, el in zip(recs, v.eligible):
            if r.flag & 1:
                assert not el
                continue
            tl.write_sam(sam, refs, [r])
            st = oracle.pss(g, sam, o)[2]
            assert bool(st[tl.ST_OK]) == bool(el), r
            if el:
                tl.write_sam(sam, refs, dl.flag_recs([r], [True]))
                st2 = oracle.pss(g, sam, o)[2]
                assert int(st2[tl.ST_OK]) == 0 and int(st2[tl.ST_FILTERED]) == 1, r
                seen.add(True)
        assert seen and 0 < v.totals["flagged"] < v.totals["eligible"] < len(recs)
    finally:
        oracle.free_genome(g)


def test_eligibility_is_fragkons_candidate_test_record_by_record(oracle, tmp_path):
    contigs, refs, recs = fuzz(5103, 400)
    o = tl.FkOpts(klen=4, min_mq=10, min_read_len=5, max_read_len=200)
    v = dl.judge_recs(recs, setup_of(contigs, refs, fk=o))
    fa, sam = tmp_path / "g.fa", tmp_path / "one.sam"
    tl.write_fasta(fa, contigs)
    g = oracle.load_genome(fa)
    try:
        for r, el in zip(recs, v.eligible):
            if r.flag & 1:
                continue
            tl.write_sam(sam, refs, [r])
            st = oracle.fragkon(g, sam, o)[2]
            # (a candidate whose window holds a non-ACGT base fails its add: KMER_FAIL, still a candidate)
            assert bool(st[tl.ST_OK] + st[tl.ST_KMER_FAIL]) == bool(el), r
        assert 0 < v.totals["flagged"]
    finally:
        oracle.free_genome(g)


def test_first_in_input_order_wins_and_only_eligible_records_shadow():
    refs, contigs = [("c", 1000)], {"c": 1000}
    s = dl.Setup(refs, contigs, pss=tl.PssOpts(region_len=5, min_mq=30))
    seq = "ACGTACGTAC"
    mk = lambda name, **kw: tl.Rec(**{**dict(qname=name, flag=0, rname="c", pos=101, mapq=40, cigar=[(10, "M")], seq=seq, qual="I" * 10), **kw})  # noqa: E731
    recs = [mk("lowmq", mapq=3), mk("secondary", flag=0x100), mk("clipped", cigar=[(2, "S"), (8, "M")]), mk("flagged", flag=0x400),
            mk("paired", flag=0x43, tlen=10), mk("first"), mk("dup1"), mk("rev", flag=0x10), mk("dup2"), mk("rev_dup", flag=0x10),
            mk("shorter", seq=seq[:9], qual="I" * 9, cigar=[(9, "M")]), mk("paired2", flag=0x83, tlen=10), mk("elsewhere", pos=102)]
    v = dl.judge_recs(recs, s)
    assert [r.qname for r, d in zip(recs, v.dup) if d] == ["dup1", "dup2", "rev_dup"]
    assert [r.qname for r, e in zip(recs, v.eligible) if e] == ["first", "dup1", "rev", "dup2", "rev_dup", "shorter", "elsewhere"]
    assert v.totals == {"eligible": 7, "distinct": 4, "flagged": 3}
    assert [int(x) for x in v.hist[:4]] == [0, 2, 1, 1] and int(v.hist.sum()) == 4


def test_read_groups_make_keys_and_R_makes_eligibility():
    refs, contigs = [("c", 1000)], {"c": 1000}
    mk = lambda name, rg: tl.Rec(qname=name, flag=0, rname="c", pos=50, mapq=40, cigar=[(8, "M")], seq="ACGTACGT", qual="I" * 8,  # noqa: E731
                                 tags=[("RG", "Z", rg)] if rg else [])
    recs = [mk("a1", "A"), mk("b1", "B"), mk("a2", "A"), mk("n1", None), mk("x1", "X"), mk("b2", "B")]
    plain = dl.judge_recs(recs, dl.Setup(refs, contigs, pss=tl.PssOpts(region_len=3)))
    assert plain.totals == {"eligible": 6, "distinct": 1, "flagged": 5}
    grouped = dl.judge_recs(recs, dl.Setup(refs, contigs, pss=tl.PssOpts(region_len=3), groups=["A", "B"]))
    assert [r.qname for r, d in zip(recs, grouped.dup) if d] == ["a2", "x1", "b2"]   # (n1 and x1 share the unassigned bucket)
    only_b = dl.judge_recs(recs, dl.Setup(refs, contigs, pss=tl.PssOpts(region_len=3), read_group="B"))
    assert [r.qname for r, d in zip(recs, only_b.dup) if d] == ["b2"] and only_b.totals["eligible"] == 2


def test_raw_and_rec_views_agree():
    contigs, refs, recs = fuzz(5104, 400, with_rg=True)
    s = setup_of(contigs, refs, pss=tl.PssOpts(region_len=6, min_mq=10), groups=["grpA", "grpB"])
    a, raw = dl.judge_recs(recs, s), tl.raw_records(refs, recs)
    b = dl.judge_raw(raw, s)
    assert np.array_equal(a.eligible, b.eligible) and np.array_equal(a.dup, b.dup) and a.totals == b.totals
    flagged = dl.flag_raw(raw, a.dup)
    assert bytes(flagged) == bytes(tl.raw_records(refs, dl.flag_recs(recs, a.dup))) and a.totals["flagged"] > 0


@pytest.mark.skipif(not tl.have_ref(), reason="oracle/_ref is not built (the reference's sources are not on this machine)")
def test_the_reference_on_the_flagged_input_is_the_oracle_on_it(oracle, tmp_path):
    contigs, refs, recs = fuzz(5105, 600)
    o = tl.PssOpts(region_len=8, min_mq=15)
    v = dl.judge_recs(recs, setup_of(contigs, refs, pss=o))
    flagged = tl.ref_safe(dl.flag_recs(recs, v.dup))
    fa, sam = tmp_path / "g.fa", tmp_path / "f.sam"
    tl.write_fasta(fa, contigs)
    tl.write_sam(sam, refs, flagged)
    fwd, rev, *_ = tl.run_ref_pss(fa, sam, tmp_path / "ref", o)
    g = oracle.load_genome(fa)
    try:
        ofwd, orev, _ = oracle.pss(g, sam, o)
    finally:
        oracle.free_genome(g)
    assert np.array_equal(fwd, ofwd) and np.array_equal(rev, orev) and v.totals["flagged"] > 0


# ---- the report writer -----------------------------------------------------------------------------------------------------------

def test_report_writer_matches_the_golden_file(host, tmp_path):
    setup, raw = dl.golden_input()
    v = dl.judge_raw(raw, setup)
    assert v.totals["flagged"] > 100 and int(v.hist[2]) > 0 and int(v.hist[3]) > 0
    totals = (C.c_uint64 * 3)(v.totals["eligible"], v.totals["distinct"], v.totals["flagged"])
    hist = (C.c_uint64 * (dl.HIST_MAX + 2))(*[int(x) for x in v.hist])
    assert host.pss_write_duplicates(b"setD.fa", b"setD.dup.bam", str(tmp_path / "out").encode(), b"pss", totals, hist, dl.HIST_MAX) == 0
    got = (tmp_path / "out.pss.duplicates.txt").read_bytes()
    assert got == (dl.GOLD / "duplicates_setD.txt").read_bytes()
    assert got.decode() == dl.report_text("setD.fa", "setD.dup.bam", v.totals, v.hist)
    assert [p.name for p in tmp_path.iterdir()] == ["out.pss.duplicates.txt"]


def test_report_writer_small_limit_large_counts_and_unwritable_prefix(host, tmp_path):
    totals = (C.c_uint64 * 3)(2 ** 40 + 7, 2 ** 40, 7)
    hist = (C.c_uint64 * 4)(0, 2 ** 40 - 2, 1, 1)
    assert host.pss_write_duplicates(b"f", b"b", str(tmp_path / "o").encode(), b"fragkon", totals, hist, 2) == 0
    lines = (tmp_path / "o.fragkon.duplicates.txt").read_text().splitlines()
    assert lines[3:] == [f"eligible_reads\t{2 ** 40 + 7}", f"distinct_keys\t{2 ** 40}", "flagged_reads\t7", "duplicate_fraction\t0.000000",
                         "size\tgroups", f"1\t{2 ** 40 - 2}", "2\t1", ">2\t1"]
    zero = (C.c_uint64 * 3)(0, 0, 0)
    assert host.pss_write_duplicates(b"f", b"b", str(tmp_path / "z").encode(), b"pss", zero, (C.c_uint64 * 4)(), 2) == 0
    assert "duplicate_fraction\t0.000000" in (tmp_path / "z.pss.duplicates.txt").read_text()
    assert host.pss_write_duplicates(b"f", b"b", str(tmp_path / "no_such_dir" / "o").encode(), b"pss", totals, hist, 2) == 1


# ---- the C ABI and the command lines ---------------------------------------------------------------------------------------------

def test_duplicates_symbols_are_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_duplicates", "pssbam_engine_finish_duplicates"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert pkg.MAX_DUP_HIST == 65535
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_MAX_DUP_HIST 65535\b", hdr)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert re.search(r"int pssbam_engine_set_duplicates\(pssbam_engine \*e, int32_t on, uint32_t initial_slots\);", hdr)
    assert re.search(r"int pssbam_engine_finish_duplicates\(pssbam_engine \*e, uint64_t totals\[3\], uint64_t \*hist, int32_t hist_max\);", hdr)
    assert L.pssbam_engine_set_duplicates(None, 1, 0) == -1      # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_duplicates(None, None, None, 255) == -1


def _run_cli(tool, tmp_path, *args, env=None):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / tool
    import os
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"), *args],
                          capture_output=True, text=True, timeout=60, env={**os.environ, **(env or {})})


@pytest.mark.parametrize("args", [["-d", "-I"], ["-I", "-d"]])
def test_cli_refuses_d_with_I_before_any_work(tmp_path, args):
    pr = _run_cli("pss-bam", tmp_path, *args)
    assert pr.returncode == 1
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-d" in lines[0] and "-I" in lines[0] and "does not go with" in lines[0], pr.stderr
    assert "Unknown option" not in pr.stderr and not list(tmp_path.iterdir())


@pytest.mark.parametrize("tool", ["pss-bam", "fragkon"])
def test_cli_refuses_d_on_several_gpus_before_any_work(tmp_path, tool):
    pr = _run_cli(tool, tmp_path, "-d", env={"PSSBAM_NGPU": "2"})
    assert pr.returncode == 1
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-d" in lines[0] and "PSSBAM_NGPU=2" in lines[0] and "Full command" not in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("tool", ["pss-bam", "fragkon"])
def test_cli_knows_d(tool):
    pkg = ge.load_pkg()
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / tool), "-d"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "Unknown option" not in pr.stderr and "-d <flag duplicates" in pr.stderr

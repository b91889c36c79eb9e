"""Depth of coverage of the tallied reads (pss-bam -c / -b) without a GPU: the Python restatement of the definition (coverage_lib)
against the CPU oracle and the unmodified reference, the two writers of libpssbam_host.so against the committed golden files, the
C-ABI symbols, and the command lines' refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import coverage_lib as cl
import duplicates_lib as dl
import pssbam_testlib as tl

# every base letter a fuzz contig holds is in both context sets: the oracle then tallies exactly the candidates
ALL_CTX = "ACGTNRYMKSWBDHV"


def setup_of(contigs, refs, **kw):
    return dl.Setup(refs, {n: len(s) for n, s in contigs}, **kw)


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.pss_write_coverage.restype = C.c_int
    L.pss_write_coverage.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_uint8), u64p, u64p, u64p, C.c_int]
    L.pss_write_coverage_bedgraph.restype = C.c_int
    L.pss_write_coverage_bedgraph.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(C.c_int32), u32p, u32p, u32p]
    return L


def write_summary(host, prefix, refs, contigs, s, fasta=b"setD.fa", bam=b"setD.bam", hist_max=cl.HIST_MAX):
    n = len(refs)
    names = (C.c_char_p * n)(*[nm.encode() for nm, _ in refs])
    held = (C.c_uint8 * n)(*[1 if nm in contigs else 0 for nm, _ in refs])
    lens = (C.c_uint64 * n)(*[contigs.get(nm, 0) for nm, _ in refs])
    per = (C.c_uint64 * (3 * n))(*[int(v) for v in s.per_contig.reshape(-1)])
    hist = (C.c_uint64 * (hist_max + 2))(*[int(v) for v in s.hist])
    return host.pss_write_coverage(fasta, bam, str(prefix).encode(), n, names, held, lens, per, hist, hist_max)


def write_bedgraph(host, path, refs, runs):
    n, m = len(refs), len(runs[0])
    names = (C.c_char_p * n)(*[nm.encode() for nm, _ in refs])
    arr = lambda t, v: (t * max(m, 1))(*[int(x) for x in v])  # noqa: E731
    return host.pss_write_coverage_bedgraph(str(path).encode(), n, names, m, arr(C.c_int32, runs[0]), arr(C.c_uint32, runs[1]), arr(C.c_uint32, runs[2]),
                                            arr(C.c_uint32, runs[3]))


# ---- the model against the oracle ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [7101, 7102])
def test_a_record_alone_gives_depth_one_over_its_span_iff_the_oracle_tallies_it(oracle, tmp_path, seed):
    contigs, refs, recs = tl.fuzz_dataset(seed, 500)
    o = tl.PssOpts(region_len=4, min_mq=20, min_read_len=10, max_read_len=120, up_ctx=ALL_CTX, down_ctx=ALL_CTX)
    s = setup_of(contigs, refs, pss=o)
    idx = {n: i for i, (n, _) in enumerate(refs)}
    fa, sam = tmp_path / "g.fa", tmp_path / "one.sam"
    tl.write_fasta(fa, contigs)
    g = oracle.load_genome(fa)
    seen = {"kept": 0, "dropped": 0, "paired_kept": 0, "paired_dropped": 0}
    try:
        for r in recs:
            tl.write_sam(sam, refs, [r])
            st = oracle.pss(g, sam, o)[2]
            c = cl.core_of_rec(r, idx)
            k = cl.kept(c, s)
            assert bool(st[tl.ST_OK]) == k, r
            seen[("paired_" if r.flag & 1 else "") + ("kept" if k else "dropped")] += 1
            got = cl.from_recs([r], s)
            if not k:
                assert got.n_runs == 0 and int(got.per_contig.sum()) == 0
                continue
            ref, pos0, L = cl.span(c)
            assert L == (abs(r.tlen) if r.flag & 1 else len(r.seq))
            assert [tuple(int(v[0]) for v in got.runs)] == [(ref, pos0, pos0 + L, 1)]
            assert [int(v) for v in got.per_contig[ref]] == [L, L, 1] and int(got.hist[1]) == L and int(got.hist[2:].sum()) == 0
            d = got.depths[ref]
            assert d[pos0:pos0 + L].min() == 1 and d.sum() == L
        assert all(seen.values()), seen
    finally:
        oracle.free_genome(g)


def test_raw_and_rec_views_agree_and_overlaps_add_up():
    contigs, refs, recs = tl.fuzz_dataset(7103, 600)
    s = setup_of(contigs, refs, pss=tl.PssOpts(region_len=6, min_mq=10))
    idx = {n: i for i, (n, _) in enumerate(refs)}
    keep = [r for r in recs if cl.kept(cl.core_of_rec(r, idx), s)]
    a = cl.from_recs(recs, s)
    b = cl.from_raw(tl.raw_records(refs, keep), refs, s.contigs)
    assert cl.same(a, b.per_contig, b.hist, b.runs) and a.n_runs > 50 and int(a.hist[2:].sum()) > 0
    # the summary's own identities
    total = sum(c for n, c in s.contigs.items() if n in {r for r, _ in refs})
    assert int(a.hist.sum()) == total and int(a.per_contig[:, 0].sum()) == total - int(a.hist[0])
    assert int(a.per_contig[:, 1].sum()) == sum(cl.span(cl.core_of_rec(r, idx))[2] for r in keep)
    ref, st, en, dp = a.runs
    assert np.all(en > st) and np.all(dp > 0) and int(((en - st).astype(np.int64) * dp).sum()) == int(a.per_contig[:, 1].sum())
    touching = (ref[1:] == ref[:-1]) & (st[1:] == en[:-1])
    assert touching.any() and np.all(dp[1:][touching] != dp[:-1][touching])       # maximal: runs that touch differ in depth
    order = np.lexsort((st, ref))
    assert np.array_equal(order, np.arange(len(ref)))


def test_depth_above_255_and_a_contig_the_genome_lacks():
    refs, contigs = [("a", 40), ("missing", 99), ("b", 30)], {"a": 40, "b": 30, "extra": 10}
    spans = [(0, 5, 10)] * 300 + [(2, 2, 26), (2, 10, 5)]
    s = cl.from_spans(spans, refs, contigs)
    assert [int(v) for v in s.per_contig.reshape(-1)] == [10, 3000, 300, 0, 0, 0, 26, 31, 2]
    assert int(s.hist[0]) == 30 + 4 and int(s.hist[256]) == 10 and int(s.hist[1]) == 21 and int(s.hist[2]) == 5 and int(s.hist.sum()) == 70
    assert [tuple(int(x) for x in r) for r in zip(*s.runs)] == [(0, 5, 15, 300), (2, 2, 10, 1), (2, 10, 15, 2), (2, 15, 28, 1)]
    text = cl.coverage_text("f", "b", refs, contigs, s)
    assert "missing" not in text and "a\t40\t10\t0.250000\t3000\t75.000000\t300\n" in text and "total\t70\t36\t0.514286\t3031\t43.300000\t300\n" in text
    assert text.endswith("255\t0\n>255\t10\n")


@pytest.mark.skipif(not tl.have_ref(), reason="oracle/_ref is not built (the reference's sources are not on this machine)")
def test_the_reference_tallies_exactly_the_kept_records(oracle, tmp_path):
    """the unmodified reference on the whole input equals itself on the records the model keeps: the tables hold those reads alone"""
    contigs, refs, recs = tl.fuzz_dataset(7104, 600)
    recs = tl.ref_safe(recs)
    o = tl.PssOpts(region_len=8, min_mq=15, up_ctx=ALL_CTX, down_ctx=ALL_CTX)
    s = setup_of(contigs, refs, pss=o)
    idx = {n: i for i, (n, _) in enumerate(refs)}
    keep = [r for r in recs if cl.kept(cl.core_of_rec(r, idx), s)]
    assert 0 < len(keep) < len(recs)
    fa, all_sam, kept_sam = tmp_path / "g.fa", tmp_path / "all.sam", tmp_path / "kept.sam"
    tl.write_fasta(fa, contigs)
    tl.write_sam(all_sam, refs, recs)
    tl.write_sam(kept_sam, refs, keep)
    fwd, rev, *_ = tl.run_ref_pss(fa, all_sam, tmp_path / "ref_all", o)
    kfwd, krev, *_ = tl.run_ref_pss(fa, kept_sam, tmp_path / "ref_kept", o)
    assert np.array_equal(fwd, kfwd) and np.array_equal(rev, krev) and int(fwd.sum()) > 0
    g = oracle.load_genome(fa)
    try:
        assert int(oracle.pss(g, kept_sam, o)[2][tl.ST_OK]) == len(keep)
    finally:
        oracle.free_genome(g)


# ---- the writers -----------------------------------------------------------------------------------------------------------------

def test_writers_match_the_golden_files(host, tmp_path):
    refs, contigs, spans = cl.kept_of_golden()
    s = cl.from_spans(spans, refs, contigs)
    assert s.n_runs > 100 and int(s.hist[3:].sum()) > 0
    assert write_summary(host, tmp_path / "out", refs, contigs, s) == 0
    got = (tmp_path / "out.pss.coverage.txt").read_bytes()
    assert got == (cl.GOLD / "coverage_setD.txt").read_bytes()
    assert got.decode() == cl.coverage_text("setD.fa", "setD.bam", refs, contigs, s)
    assert write_bedgraph(host, tmp_path / "out.bedgraph", refs, s.runs) == 0
    bg = (tmp_path / "out.bedgraph").read_bytes()
    assert bg == (cl.GOLD / "coverage_setD.bedgraph").read_bytes() and bg.decode() == cl.bedgraph_text(refs, s.runs)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.bedgraph", "out.pss.coverage.txt"]       # (no .tmp stays)


def test_writers_small_limit_large_counts_empty_and_unwritable_prefix(host, tmp_path):
    refs, contigs = [("c", 2 ** 33), ("gone", 5), ("e", 0)], {"c": 2 ** 33, "e": 0}
    s = cl.Summary(np.array([[2 ** 32 + 1, 2 ** 40, 2 ** 32 - 1], [0, 0, 0], [0, 0, 0]], dtype=np.uint64),
                   np.array([2 ** 33 - 2 ** 32 - 1, 2 ** 32, 0, 1], dtype=np.uint64), (np.zeros(0),) * 4, [])
    assert write_summary(host, tmp_path / "o", refs, contigs, s, b"f", b"b", hist_max=2) == 0
    lines = (tmp_path / "o.pss.coverage.txt").read_text().splitlines()
    assert lines[3:] == ["contig\tlength\tcovered_bases\tbreadth\tdepth_sum\tmean_depth\tmax_depth",
                         f"c\t{2 ** 33}\t{2 ** 32 + 1}\t0.500000\t{2 ** 40}\t128.000000\t{2 ** 32 - 1}", "e\t0\t0\t0.000000\t0\t0.000000\t0",
                         f"total\t{2 ** 33}\t{2 ** 32 + 1}\t0.500000\t{2 ** 40}\t128.000000\t{2 ** 32 - 1}", "depth\tpositions",
                         f"0\t{2 ** 33 - 2 ** 32 - 1}", f"1\t{2 ** 32}", "2\t0", ">2\t1"]
    assert lines[:3] == [cl.coverage_text("f", "b", refs, contigs, s, 2).splitlines()[0], "# FASTA: f", "# BAM: b"]
    assert write_summary(host, tmp_path / "no_such_dir" / "o", refs, contigs, s, hist_max=2) == 1
    # the bedGraph: empty is a file; an unwritable place and a run outside the names leave nothing behind
    assert write_bedgraph(host, tmp_path / "empty.bedgraph", refs, (np.zeros(0),) * 4) == 0 and (tmp_path / "empty.bedgraph").read_bytes() == b""
    assert write_bedgraph(host, tmp_path / "no_such_dir" / "x.bedgraph", refs, ([0], [1], [2], [3])) == 1
    assert write_bedgraph(host, tmp_path / "bad.bedgraph", refs, ([0, 7], [1, 1], [2, 2], [3, 3])) == 1
    assert sorted(p.name for p in tmp_path.iterdir()) == ["empty.bedgraph", "o.pss.coverage.txt"]


# ---- the C ABI and the command lines ---------------------------------------------------------------------------------------------

def test_coverage_symbols_are_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_coverage", "pssbam_engine_finish_coverage", "pssbam_engine_finish_coverage_runs"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert pkg.COV_HIST_MAX == 255
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_COV_HIST_MAX 255\b", hdr)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert re.search(r"int pssbam_engine_set_coverage\(pssbam_engine \*e, int32_t on, uint64_t positions_hint\);", hdr)
    assert re.search(r"int pssbam_engine_finish_coverage\(pssbam_engine \*e, int32_t first_ref, int32_t n, uint64_t \*per_contig, uint64_t \*hist, "
                     r"int32_t hist_max,\s+uint64_t \*n_runs\);", hdr)
    assert re.search(r"int pssbam_engine_finish_coverage_runs\(pssbam_engine \*e, uint64_t cap, int32_t \*ref, uint32_t \*start, uint32_t \*end, "
                     r"uint32_t \*depth,\s+uint64_t \*n_runs\);", hdr)
    assert L.pssbam_engine_set_coverage(None, 1, 0) == -1      # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_coverage(None, 0, 0, None, None, 255, None) == -1
    assert L.pssbam_engine_finish_coverage_runs(None, 0, None, None, None, None, None) == -1


def _run_cli(tool, tmp_path, *args, env=None):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / tool
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"), *args],
                          capture_output=True, text=True, timeout=60, env={**os.environ, **(env or {})})


def _one_line(pr, tmp_path):
    assert pr.returncode == 1
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "Unknown option" not in pr.stderr and "Full command" not in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())
    return lines[0]


@pytest.mark.parametrize("args", [["-c", "-I"], ["-I", "-c"], ["-I", "-b", "x.bedgraph"], ["-b", "x.bedgraph", "-I"]])
def test_cli_refuses_coverage_with_I_before_any_work(tmp_path, args):
    line = _one_line(_run_cli("pss-bam", tmp_path, *args), tmp_path)
    assert ("-c" in line or "-b" in line) and "-I" in line and "does not go with" in line


@pytest.mark.parametrize("args", [["-c"], ["-b", "x.bedgraph"]])
def test_cli_refuses_coverage_on_several_gpus_before_any_work(tmp_path, args):
    line = _one_line(_run_cli("pss-bam", tmp_path, *args, env={"PSSBAM_NGPU": "2"}), tmp_path)
    assert args[0] in line and "PSSBAM_NGPU=2" in line


def test_cli_refuses_b_naming_the_input_or_the_kept_bam(tmp_path):
    line = _one_line(_run_cli("pss-bam", tmp_path, "-b", str(tmp_path / "none.bam")), tmp_path)
    assert "-b must not name" in line and "-B" in line
    line = _one_line(_run_cli("pss-bam", tmp_path, "-O", str(tmp_path / "kept.bam"), "-b", str(tmp_path / "kept.bam")), tmp_path)
    assert "-b must not name" in line and "-O" in line
    line = _one_line(_run_cli("pss-bam", tmp_path, "-b", str(tmp_path / "no_such_dir" / "x.bedgraph")), tmp_path)
    assert "-b: cannot create" in line


@pytest.mark.parametrize("args", [["-c"], ["-b", "x.bedgraph"]])
def test_fragkon_has_neither(tmp_path, args):
    line = _one_line(_run_cli("fragkon", tmp_path, *args), tmp_path)
    assert args[0] in line and "pss-bam" in line


def test_cli_knows_c_and_b():
    pkg = ge.load_pkg()
    for args in (["-c"], ["-b", "x.bedgraph"]):
        pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), *args], capture_output=True, text=True, timeout=60)
        assert pr.returncode == 1 and "Unknown option" not in pr.stderr
        assert "-c <also write the depth of coverage" in pr.stderr and "-b <out.bedgraph>" in pr.stderr

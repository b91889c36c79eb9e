"""pss-bam -T / fragkon -T without a GPU: the C ABI carries the setter, both command lines know the option and refuse a
bad BED file before any GPU work, and the yardstick the GPU tests use -- the CPU oracle on the input reduced to the
records `samtools view -L` keeps (regions_lib) -- is itself checked against a direct count that restates the filters
and skips the reads no region covers.  The usage text of both tools is the reference's and stays as it is (as for
-G / -S / -C / -Q); the lines that present -T are README's, one per tool."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import pssbam_testlib as tl
import regions_lib as rl

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_pkg()


def test_setter_is_declared_listed_and_exported(pkg):
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^#define PSSBAM_MAX_REGIONS \(1 << 26\)", hdr, re.M)
    assert re.search(r"^int pssbam_engine_set_regions\(pssbam_engine \*e, int32_t n_names, const char \*const \*names, int64_t n_regions,\n"
                     r"\s+const int32_t \*name_of, const uint32_t \*starts, const uint32_t \*ends\);$", hdr, re.M)
    assert "pssbam_engine_set_regions" in pkg.HIP_SYMBOLS and pkg.MAX_REGIONS == 1 << 26
    assert callable(pkg.Engine.set_regions)
    L = pkg.hip_lib()
    f = L.pssbam_engine_set_regions
    f.restype = C.c_int
    L.pssbam_last_error.restype = C.c_char_p
    assert f(None, 0, None, 0, None, None, None) == -1     # PSSBAM_EINVAL, not a dereference
    assert L.pssbam_last_error()


def test_abi_structs_keep_their_layout(pkg):
    """-T adds an entry point, not a field: the option structs, the stats slots and the ABI version stay as they were"""
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    pss = hdr[hdr.index("typedef struct pssbam_pss_opts"):hdr.index("} pssbam_pss_opts;")]
    assert re.findall(r"(\w+);", pss) == ["region_len", "min_read_len", "max_read_len", "min_mq", "up_ctx", "down_ctx",
                                          "merged_only"]
    kmer = hdr[hdr.index("typedef struct pssbam_kmer_opts"):hdr.index("} pssbam_kmer_opts;")]
    assert re.findall(r"(\w+);", kmer) == ["klen", "min_mq", "min_read_len", "max_read_len", "merged_only"]
    cfg = hdr[hdr.index("typedef struct pssbam_config"):hdr.index("} pssbam_config;")]
    assert re.findall(r"(\w+);", cfg) == ["abi_version", "tally_mask", "pss", "kmer", "read_group", "device", "kernel"]
    assert re.search(r"PSSBAM_ST_SLOW_PATH = 9,", hdr) and re.search(r"PSSBAM_ST_N = 16\b", hdr) and len(pkg.ST_NAMES) == 10   # no new stats slot


@pytest.mark.parametrize("tool", ["pss-bam", "fragkon"])
def test_T_is_a_known_option_and_readme_presents_it(pkg, tool):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / tool), "-T", "x.bed"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "Unknown option" not in pr.stderr          # no -F / -B: the usage text
    assert pr.stderr.startswith("pss-bam v1.2.1" if tool == "pss-bam" else "fragkon: Program")
    readme = (ROOT / "README.md").read_text()
    assert re.search(rf"^pss-bam_amd/bin/{tool} .* -T \S+\.bed", readme, re.M)


def run_cli(pkg, tool, tmp_path, bed_text, name="r.bed"):
    bed = tmp_path / name
    if bed_text is not None:
        bed.write_bytes(bed_text if isinstance(bed_text, bytes) else bed_text.encode())
    args = [str(pkg.PKG_DIR / "bin" / tool), "-F", str(tmp_path / "no.fa"), "-B", str(tmp_path / "no.bam"), "-T", str(bed)]
    if tool == "pss-bam":
        args += ["-o", str(tmp_path / "out")]
    return subprocess.run(args, capture_output=True, text=True, timeout=60)


BAD_BED = [
    ("chrA\tx\t10\n", "line 1"), ("chrA\t1\t1e3\n", "line 1"), ("# c\nchrA\t-1\t10\n", "line 2"), ("chrA\t1.5\t10\n", "line 1"),
    ("chrA\t0\t10\nchrA\t4294967296\t4294967297\n", "line 2"), ("chrA\t5\t4294967296\n", "line 1"),
    ("chrA\t0\t99999999999999999999999\n", "line 1"), ("\n\nchrA\t10\t9\n", "line 3"), ("chrA\t10\n", "line 1"),
    ("", "no usable"), ("# only\ntrack x\nbrowser y\n\n", "no usable"), ("chrA\t7\t7\n", "no usable"), (None, "r.bed"),
    (b"\x1f\x8b\x08\x00rest", "plain-text"),
]


@pytest.mark.parametrize("tool", ["pss-bam", "fragkon"])
@pytest.mark.parametrize("text,what", BAD_BED)
def test_cli_refuses_bad_bed_before_any_work(pkg, tool, text, what, tmp_path):
    pr = run_cli(pkg, tool, tmp_path, text)
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    lines = pr.stderr.splitlines()
    assert len(lines) == 1 and "-T" in lines[0] and what in lines[0] and "r.bed" in lines[0], pr.stderr
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr and "Entered command" not in pr.stderr
    assert pr.stdout == "" and [p.name for p in tmp_path.iterdir()] in ([], ["r.bed"])


GOOD_BED = [
    "chrA\t0\t10\n", "chrA 0 10\n", "  chrA \t 0  10  name 0 +\n", "chrA\t0\t10", "chrA\t0\t10\r\n", "chrA\t0\t4294967295\n",
    "track name=x\nbrowser position chrA:1-5\n#c\n\nchrA\t5\t5\nchrA\t3\t9\nchrA\t3\t9\nchrB\t1\t2\n",
]


@pytest.mark.parametrize("tool", ["pss-bam", "fragkon"])
@pytest.mark.parametrize("text", GOOD_BED)
def test_cli_accepts_bed_forms(pkg, tool, text, tmp_path):
    """an accepted BED lets the command go on to its next step: the missing FASTA (still before any GPU call)"""
    pr = run_cli(pkg, tool, tmp_path, text)
    assert "-T" not in pr.stderr.replace(f"-T {tmp_path / 'r.bed'}", ""), pr.stderr
    assert "no.fa" in pr.stderr and pr.returncode != 0


def test_host_parser(pkg):
    class Regions(C.Structure):
        _fields_ = [("n_names", C.c_int32), ("names", C.POINTER(C.c_char_p)), ("n", C.c_int64), ("name_of", C.POINTER(C.c_int32)),
                    ("starts", C.POINTER(C.c_uint32)), ("ends", C.POINTER(C.c_uint32))]
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_bed.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Regions), C.c_char_p, C.c_size_t]
    L.pss_free_regions.argtypes = [C.POINTER(Regions)]
    text = b"track t\nchr2 5 9\nchr1\t0\t3\textra\n# c\nchr2\t100\t4294967295\nchr1\t3\t3\n"
    r, err = Regions(), C.create_string_buffer(200)
    assert L.pss_parse_bed(text, len(text), C.byref(r), err, 200) == 0
    assert [r.names[i] for i in range(r.n_names)] == [b"chr2", b"chr1"]
    got = [(r.name_of[i], r.starts[i], r.ends[i]) for i in range(r.n)]
    assert got == [(0, 5, 9), (1, 0, 3), (0, 100, 4294967295), (1, 3, 3)]
    L.pss_free_regions(C.byref(r))
    assert L.pss_parse_bed(b"a\t2\t1\n", 6, C.byref(r), err, 200) == -1 and b"line 1" in err.value


# ---- the yardstick ---------------------------------------------------------------------------------------------------

def test_keep_rec_is_the_samtools_rule():
    reg = rl.regions_dict([("c", 10, 20), ("c", 30, 30), ("d", 0, 5)])
    def rec(pos, cigar, rname="c"):
        return tl.Rec("q", 0, rname, pos, 30, cigar)
    assert not rl.keep_rec(rec(6, [(5, "M")]), reg)            # [5, 10): ends at the start -- touching is not overlapping
    assert rl.keep_rec(rec(6, [(6, "M")]), reg)                # [5, 11): one shared base
    assert rl.keep_rec(rec(20, [(9, "M")]), reg)               # [19, 28): one shared base
    assert not rl.keep_rec(rec(21, [(9, "M")]), reg)           # [20, 29): starts at the end
    assert not rl.keep_rec(rec(26, [(10, "M")]), reg)          # the empty interval [30, 30) keeps nothing
    assert rl.keep_rec(rec(4, [(2, "M"), (8, "D"), (2, "M")]), reg) and not rl.keep_rec(rec(4, [(2, "M"), (8, "I"), (2, "M")]), reg)
    assert rl.keep_rec(rec(15, []), reg) and not rl.keep_rec(rec(21, []), reg)      # no CIGAR: one base
    assert not rl.keep_rec(rec(12, [(5, "M")], "e"), reg) and rl.keep_rec(rec(1, [(1, "M")], "d"), reg)
    text = "@SQ\tSN:c\tLN:90\nr\t0\tc\t6\t9\t5M\t*\t0\t0\tACGTA\t*\nq\t0\tc\t6\t9\t6M\t*\t0\t0\tACGTAC\t*\n"
    assert rl.reduce_sam_text(text, [("c", 10, 20)]) == "@SQ\tSN:c\tLN:90\nq\t0\tc\t6\t9\t6M\t*\t0\t0\tACGTAC\t*\n"


fuzz_case = rl.fuzz_case


def non_vacuous(oracle, tmp_path, contigs, refs, recs, ivs, tag):
    """of the records the unfiltered oracle tallies (pss at -r 15; fragkon at k = 4 and 8), the regions keep >= 10 % and
    drop >= 10 %"""
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        for name, rs in (("all", recs), ("safe", tl.ref_safe(recs, 8))):
            plain, red = tmp_path / f"{tag}_{name}.sam", tmp_path / f"{tag}_{name}_red.sam"
            tl.write_sam(plain, refs, rs)
            rl.write_reduced_sam(red, refs, rs, ivs)
            runs = [(oracle.pss, tl.PssOpts(region_len=15)), (oracle.fragkon, tl.FkOpts(klen=4)), (oracle.fragkon, tl.FkOpts(klen=8))]
            for fn, o in runs:
                n_all, n_kept = int(fn(g, plain, o)[2][tl.ST_OK]), int(fn(g, red, o)[2][tl.ST_OK])
                assert n_kept >= 0.1 * n_all and n_all - n_kept >= 0.1 * n_all, (tag, name, o, n_all, n_kept)
    finally:
        oracle.free_genome(g)


@pytest.mark.parametrize("seed", rl.PSS_SEEDS + rl.FK_SEEDS + rl.RG_SEEDS)
def test_every_fuzz_case_keeps_and_drops_a_tenth(oracle, tmp_path, seed):
    contigs, refs, recs, ivs = fuzz_case(seed)
    non_vacuous(oracle, tmp_path, contigs, refs, recs, ivs, f"s{seed}")


def test_many_refs_cases_keep_and_drop_a_tenth(oracle, tmp_path):
    from test_gpu_contig_sets import _many_refs_dataset
    from test_gpu_many_refs import _dataset
    contigs, refs, recs = _dataset(rl.MANY_REFS_SEED, False)
    assert all(dict(refs)[nm] and [n for n, _ in refs].index(nm) >= 64 for nm, _, _ in rl.MANY_REFS_IVS)
    non_vacuous(oracle, tmp_path, contigs, refs, recs, rl.MANY_REFS_IVS, "many")
    contigs, refs, recs = _many_refs_dataset(rl.STAR_SEED)
    assert any(r.rname == "*" and rl.keep_rec(r, rl.regions_dict(rl.STAR_IVS)) and r.cigar == [(len(r.seq), "M")] for r in recs)
    non_vacuous(oracle, tmp_path, contigs, refs, recs, rl.STAR_IVS, "star")


def test_generated_intervals_hit_the_edges():
    contigs, refs, recs, ivs = fuzz_case(rl.PSS_SEEDS[0])
    reg = rl.regions_dict(ivs)
    spans = [(r.pos - 1, r.pos - 1 + r.cigar[0][0]) for r in recs if r.rname == "chrB" and len(r.cigar) == 1 and r.cigar[0][1] == "M"]
    chrB = [(s, e) for nm, s, e in ivs if nm == "chrB"]
    assert any(s == b for s, _ in chrB for _, b in spans) and any(e == a for _, e in chrB for a, _ in spans)     # touching
    assert any(s == b - 1 for s, _ in chrB for _, b in spans) and any(e == a + 1 for _, e in chrB for a, _ in spans)   # one base
    assert ("chrB", 3500, 3500) in ivs and any(s == 0 for s, _ in chrB) and any(e > 5000 for _, e in chrB)
    assert sum(1 for s, e in chrB if e - s == 1 and 3072 <= s < 4096) > 16          # one 1024-base bin
    assert any(e - s > 8 * 16 for s, e in chrB)                                       # more than 8 bins of 16 bases
    assert "scaffold_10" not in reg and "chrNowhere" in reg and not any(nm == "chrNowhere" for nm, _ in refs)
    assert any((a >> 4) != ((b - 1) >> 4) for a, b in spans)                          # reads straddle bin boundaries
    assert ivs != sorted(ivs)


@pytest.mark.parametrize("seed", rl.PSS_SEEDS)
def test_pss_oracle_on_reduced_sam_equals_direct_count(oracle, tmp_path, seed):
    """reduced SAM through the oracle == a direct count over the reads a coverage mask keeps; and the case is not
    vacuous: of the records the unfiltered oracle tallies, the regions keep >= 10 % and drop >= 10 %"""
    contigs, refs, recs, ivs = fuzz_case(seed)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        plain, red = tmp_path / "plain.sam", tmp_path / "red.sam"
        tl.write_sam(plain, refs, recs)
        kept = rl.write_reduced_sam(red, refs, recs, ivs)
        cov = rl.coverage(ivs)
        direct = [r for r in recs if rl.direct_keep(r, cov)]
        for o in (tl.PssOpts(region_len=15), tl.PssOpts(region_len=0), tl.PssOpts(region_len=16), tl.PssOpts(region_len=40),
                  tl.PssOpts(region_len=31, min_mq=10, up_ctx="CT", down_ctx="ACGTN")):
            pf, pr_, pst = oracle.pss(g, plain, o)
            rf, rr, rst = oracle.pss(g, red, o)
            df, dr = bq.direct_pss_counts(contigs, direct, o, 0)
            assert np.array_equal(rf, df) and np.array_equal(rr, dr), o
            n_all, n_kept = int(pst[tl.ST_OK]), int(rst[tl.ST_OK])
            assert n_kept >= 0.1 * n_all and n_all - n_kept >= 0.1 * n_all, (seed, o, n_all, n_kept)
            if o.region_len:
                assert not np.array_equal(pf, rf) and rf.any() and rr.any()
        if tl.have_ref():
            fa = tmp_path / "g.fa"
            tl.write_fasta(fa, contigs)
            safe = tmp_path / "safe.sam"
            tl.write_sam(safe, refs, rl.reduce_recs(tl.ref_safe(recs), ivs))
            o = tl.PssOpts(region_len=15)
            wf, wr, *_ = tl.run_ref_pss(fa, safe, tmp_path / "ref", o)
            df, dr = bq.direct_pss_counts(contigs, [r for r in tl.ref_safe(recs) if rl.direct_keep(r, cov)], o, 0)
            assert np.array_equal(wf, df) and np.array_equal(wr, dr)
        assert len(kept) < len(recs)
    finally:
        oracle.free_genome(g)


@pytest.mark.parametrize("seed", rl.FK_SEEDS)
def test_fragkon_oracle_non_vacuity(oracle, tmp_path, seed):
    """the fragkon seeds: the reduced file keeps and drops >= 10 % of the reads the unfiltered oracle adds k-mers for,
    and the reads it drops are exactly those whose [s, s + strlen(SEQ)) no region covers"""
    contigs, refs, recs, ivs = fuzz_case(seed)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        plain, red, direct = tmp_path / "plain.sam", tmp_path / "red.sam", tmp_path / "direct.sam"
        safe = tl.ref_safe(recs, 8)
        tl.write_sam(plain, refs, safe)
        rl.write_reduced_sam(red, refs, safe, ivs)
        cov = rl.coverage(ivs)
        # the direct restatement only speaks about <L>M records; every other record is never tallied, kept or not
        tl.write_sam(direct, refs, [r for r in safe if rl.direct_keep(r, cov, kmer=True) and r.cigar == [(len(r.seq), "M")]])
        for k in (4, 8):
            o = tl.FkOpts(klen=k)
            p5, p3, pst = oracle.fragkon(g, plain, o)
            r5, r3, rst = oracle.fragkon(g, red, o)
            d5, d3, _ = oracle.fragkon(g, direct, o)
            assert np.array_equal(r5, d5) and np.array_equal(r3, d3)
            n_all, n_kept = int(pst[tl.ST_OK]), int(rst[tl.ST_OK])
            assert n_kept >= 0.1 * n_all and n_all - n_kept >= 0.1 * n_all, (seed, k, n_all, n_kept)
    finally:
        oracle.free_genome(g)


def test_golden_is_what_the_reduction_gives_and_differs_from_the_unfiltered_tables(oracle, tmp_path):
    """tests/golden/regions_setA.pss.{counts,rates}.txt (recipe: test_gpu_regions.py::test_cli_T_golden): non-zero,
    different from the unfiltered pss_0 tables, and equal to the oracle on setA.sam reduced by regions_setA.bed"""
    ivs = rl.read_bed(GOLD / "regions_setA.bed")
    gf, gr = tl.parse_counts_text((GOLD / "regions_setA.pss.counts.txt").read_text())
    pf, pr_ = tl.parse_counts_text((GOLD / "pss_0.pss.counts.txt").read_text())
    assert gf.any() and gr.any() and gf[2:].any() and not np.array_equal(gf, pf) and not np.array_equal(gr, pr_)
    red = tmp_path / "setA.regions.sam"
    red.write_text(rl.reduce_sam_text((GOLD / "setA.sam").read_text(), ivs))
    g = oracle.load_genome(GOLD / "setA.fa")
    try:
        wf, wr, _ = oracle.pss(g, red, tl.PssOpts())
    finally:
        oracle.free_genome(g)
    assert np.array_equal(wf, gf) and np.array_equal(wr, gr)

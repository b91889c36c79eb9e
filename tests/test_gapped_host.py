"""pss-bam -I without a GPU: the yardstick the GPU tests use -- the CPU oracle (and, where oracle/_ref exists, the
unmodified reference) on the file with every anchoring record replaced by its anchored <span>M record -- is checked
against a direct count that walks the original CIGARs; the fuzz fixture is held to be rich enough for the GPU tests to
mean something; the C ABI and the package carry the setter; the command line refuses -I beside the options it excludes
before any work."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import gapped_lib as gl
import pssbam_testlib as tl

ROOT = Path(__file__).resolve().parent.parent
SEEDS = (9501, 9502)        # SEEDS[0] with 3000 records is the fixture of test_gpu_gapped.py
N_RECS = 3000


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_pkg()


@pytest.fixture(scope="module", params=SEEDS)
def case(request):
    return gl.fuzz_case(request.param, N_RECS)


def opts_of(seed: int, n: int) -> list:
    rng = np.random.default_rng(seed + n)
    out = [tl.PssOpts(region_len=n)]
    for _ in range(2):
        o = tl.random_pss_opts(rng)
        o.region_len = n
        out.append(o)
    return out


@pytest.mark.parametrize("n", [15, 40])
def test_oracle_on_anchored_records_equals_direct_count(oracle, case, tmp_path, n):
    contigs, refs, recs, _ = case
    sam = tmp_path / "anchored.sam"
    tl.write_sam(sam, refs, gl.anchor_recs(recs))
    plain = tmp_path / "plain.sam"
    tl.write_sam(plain, refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        for k, o in enumerate(opts_of(len(recs), n)):
            want_f, want_r = gl.direct_counts(contigs, recs, o)
            got_f, got_r, _ = oracle.pss(g, sam, o)
            assert np.array_equal(got_f, want_f) and np.array_equal(got_r, want_r), (n, o)
            if k == 0:      # and the transformation did add reads
                pf, pr, _ = oracle.pss(g, plain, o)
                assert int(got_f[1].sum()) > int(pf[1].sum()) + 100 and int(got_r[1].sum()) > int(pr[1].sum()) + 100
    finally:
        oracle.free_genome(g)


def test_anchor_rec_is_the_identity_on_len_M():
    contigs, refs, recs = tl.fuzz_dataset(SEEDS[0], 1500)
    seen = 0
    for r in recs:
        if len(r.cigar) == 1 and r.cigar[0][1] == "M":
            assert gl.anchor_rec(r) == r
            seen += gl.anchor_info(r) is not None
    assert seen > 500
    r = tl.Rec("x", 0, "chrA", 10, 30, [(3, "H"), (2, "S"), (4, "M"), (1, "I"), (2, "="), (3, "D"), (5, "X"), (1, "S")],
               seq="ttACGTaCCGGGTTc", qual="##IIII!JJKKKKK#")
    a = gl.anchor_rec(r)
    assert gl.anchor_info(r) == dict(span=14, q0=2, q1=14, a=4, b=5)
    assert (a.cigar_str(), a.seq, a.qual) == ("14M", "ACGTNNNNNGGGTT", "IIII!!!!!KKKKK")
    assert gl.anchor_sam_text(tl.sam_line(r)) == tl.sam_line(a)
    whole = tl.Rec("y", 0, "chrA", 10, 30, [(2, "S"), (3, "="), (4, "X"), (1, "H")], seq="ggACGTACG", qual="##IIIIJJJ")
    assert (gl.anchor_rec(whole).cigar_str(), gl.anchor_rec(whole).seq) == ("7M", "ACGTACG")


def test_fixture_is_not_thin(oracle, tmp_path):
    """of the 3000 records of the GPU tests' fixture: anchoring CIGARs other than <len>M, reads that -I adds at -r 40,
    short terminal runs, CIGARs beyond the tiled kernel's op cap, and enough records for at least two reasons not to anchor"""
    pkg = ge.load_pkg()
    contigs, refs, recs, why = gl.fuzz_case(SEEDS[0], N_RECS)
    assert len(recs) == N_RECS
    gapped = [r for r in recs if gl.anchor_info(r) is not None and not (len(r.cigar) == 1 and r.cigar[0][1] == "M")]
    assert len(gapped) >= 600
    o = tl.PssOpts(region_len=40)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        added = 0
        sam = tmp_path / "one.sam"
        tl.write_sam(sam, refs, gl.anchor_recs(gapped))
        _, _, st = oracle.pss(g, sam, o)
        added = int(st[tl.ST_OK])
    finally:
        oracle.free_genome(g)
    assert added >= 200
    infos = [gl.anchor_info(r) for r in gapped]
    assert sum(1 for an in infos if an["a"] < 40 or an["b"] < 40) >= 100
    assert sum(1 for r in gapped if len(r.cigar) > 8) >= 50
    assert sum(1 for r in gapped if len(r.cigar) > pkg.GAPPED_TILED_OPS) >= 10 and pkg.GAPPED_TILED_OPS >= 8
    counts = {w: sum(1 for r, x in zip(recs, why) if x == w and gl.anchor_info(r) is None) for w in gl.REASONS}
    assert all(sum(1 for x in why if x == w) == counts[w] for w in gl.REASONS)     # every broken record stays unanchored
    assert sum(1 for c in counts.values() if c >= 100) >= 2 and all(c >= 10 for c in counts.values()), counts
    # the features the generator promises
    ops_seen = {op for r in gapped for _, op in r.cigar}
    assert ops_seen >= set("MIDSH=X")
    assert any(r.cigar[0][1] == "H" and r.cigar[1][1] == "S" for r in gapped) and any(r.cigar[-1][1] == "H" and r.cigar[-2][1] == "S" for r in gapped)
    assert {an["a"] for an in infos} >= set(range(1, 31)) and max(an["b"] for an in infos) >= 60
    paired = [r for r in gapped if r.flag & 1]
    assert sum(1 for r in paired if abs(r.tlen) == r.ref_span()) >= 30 and sum(1 for r in paired if abs(r.tlen) != r.ref_span()) >= 30
    assert sum(1 for r in gapped if 12 >= sum(1 for _, op in r.cigar if op in "ID") >= 2) >= 200


@pytest.mark.skipif(not tl.have_ref(), reason="oracle/_ref is not built")
def test_reference_on_anchored_records_equals_oracle(oracle, case, tmp_path):
    contigs, refs, recs, _ = case
    fa, sam = tmp_path / "g.fa", tmp_path / "anchored.sam"
    tl.write_fasta(fa, contigs)
    safe = tl.ref_safe(gl.anchor_recs(recs))
    tl.write_sam(sam, refs, safe)
    g = oracle.load_genome(fa)
    try:
        for n in (15, 40):
            for o in opts_of(len(recs), n)[:2]:
                want_f, want_r, _ = oracle.pss(g, sam, o)
                ref_f, ref_r, _, _, _ = tl.run_ref_pss(fa, sam, tmp_path / f"ref{n}", o)
                assert np.array_equal(ref_f, want_f) and np.array_equal(ref_r, want_r), (n, o)
    finally:
        oracle.free_genome(g)


def test_setter_is_declared_listed_and_exported(pkg):
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^int pssbam_engine_set_gapped_reads\(pssbam_engine \*e, int32_t on\);$", hdr, re.M)
    L = pkg.hip_lib()
    assert "pssbam_engine_set_gapped_reads" in pkg.HIP_SYMBOLS and hasattr(L, "pssbam_engine_set_gapped_reads")
    assert L.pssbam_engine_set_gapped_reads(None, 1) == -1      # PSSBAM_EINVAL, not a dereference
    for name in ("set_gapped", "gapped"):
        assert hasattr(pkg.Engine, name)
    src = (ROOT / "pss-bam_amd" / "csrc" / "record_decode.h").read_text()
    assert re.search(rf"^constexpr uint32_t GAPPED_TILED_OPS = {pkg.GAPPED_TILED_OPS};", src, re.M)


REFUSED = [(["-I", "-G"], "-G"), (["-I", "-S", "40"], "-S"), (["-I", "-C", "map"], "-C"), (["-I", "-H", "100"], "-H"),
           (["-I", "-X", "cpg"], "-X"), (["-I", "-E", "ds"], "-E"), (["-E", "ss", "-r", "20", "-I"], "-E")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_cli_refuses_before_any_work(pkg, args, word, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(tmp_path / "no.fa"), "-B", str(tmp_path / "no.bam"), "-o", str(tmp_path / "out"), *args],
                        capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    lines = pr.stderr.splitlines()
    assert len(lines) == 1 and "-I" in lines[0] and word in lines[0] and "exclude each other" in lines[0], pr.stderr
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr
    assert pr.stdout == "" and list(tmp_path.iterdir()) == []


def test_cli_usage_names_the_option_and_fragkon_has_none(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-I"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr
    assert len([ln for ln in pr.stderr.splitlines() if ln.startswith("-I <")]) == 1
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "fragkon"), "-I"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -I." in pr.stderr

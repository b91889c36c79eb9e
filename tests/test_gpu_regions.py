"""pss-bam -T / fragkon -T on the GPU: only the reads that overlap a BED's regions are tallied.

The specification is one sentence: `-T regions.bed` on a file == the tool without -T on the same file reduced to the
records `samtools view -L regions.bed` keeps.  So every check here runs the engine (or the command) with regions on the
ORIGINAL records and compares with the CPU oracle (or the same binary, or the reference itself when oracle/_ref exists)
WITHOUT them on the reduced copy regions_lib writes (checked on its own in test_regions_host.py, which also asserts that
every case used here keeps and drops at least a tenth of the reads the unfiltered run tallies).  Each engine check runs
with PSSBAM_REGION_GRID_SHIFT 4 (16-base bins: many per contig, reads straddle them) and 10 (one or a few bins per
contig: the long in-bin searches)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import pssbam_testlib as tl
import regions_lib as rl
from test_gpu_contig_sets import _many_refs_dataset, oracle_sets
from test_gpu_kmer_planes import CLI_MODES, table_of, write_aln
from test_gpu_length_bins import bins_of, oracle_bins, pss_dict
from test_gpu_many_refs import _dataset as many_refs_dataset
from test_gpu_read_groups import first_rg

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
SHIFTS = [4, 10]
SAME = ("records", "rg_dropped", "parse_skip", "no_contig")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


class Case:
    def __init__(self, oracle, d: Path, tag, contigs, refs, recs, ivs):
        self.contigs, self.refs, self.recs, self.ivs = contigs, refs, recs, ivs
        self.raw = tl.raw_records(refs, recs)
        self.kept = rl.reduce_recs(recs, ivs)
        self.plain, self.red = d / f"{tag}.sam", d / f"{tag}.red.sam"
        tl.write_sam(self.plain, refs, recs)
        tl.write_sam(self.red, refs, self.kept)
        self.g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("regions")
    out = {seed: Case(oracle, d, f"s{seed}", *rl.fuzz_case(seed)) for seed in rl.PSS_SEEDS + rl.FK_SEEDS + rl.RG_SEEDS}
    yield out
    for c in out.values():
        oracle.free_genome(c.g)


def make_engine(pkg, c: Case, ivs, regions_first=True, **kw):
    eng = pkg.Engine(**kw)
    if ivs is not None and regions_first:
        eng.set_regions(*rl.to_arrays(ivs))
    eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
    eng.set_references([nm for nm, _ in c.refs])
    if ivs is not None and not regions_first:
        eng.set_regions(*rl.to_arrays(ivs))
    return eng


def run(pkg, c: Case, ivs, **kw):
    eng = make_engine(pkg, c, ivs, **kw)
    eng.submit(c.raw)
    return eng


def finish(eng):
    got = eng.finish()
    eng.close()
    return got


def check_stats(got: dict, plain: dict, ok_key: str, filt_key: str, n_ok: int):
    """RECORDS, RG_DROPPED, PARSE_SKIP and NO_CONTIG as without regions; a candidate that meets no region is FILTERED
    (a fragkon candidate ends as KMER_OK or KMER_FAIL: one that meets no region leaves either of them)"""
    assert {k: got[k] for k in SAME} == {k: plain[k] for k in SAME}
    assert got[ok_key] == n_ok
    fail = (lambda st: st["kmer_fail"]) if ok_key == "kmer_ok" else (lambda st: 0)
    assert got[filt_key] == plain[filt_key] + (plain[ok_key] + fail(plain)) - (got[ok_key] + fail(got))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n", [0, 15, 16, 40])
@pytest.mark.parametrize("kernel", ["SIMPLE", "TILED", "AUTO"])
def test_engine_matches_oracle_on_reduced_records(pkg, oracle, cases, monkeypatch, kernel, n, shift):
    monkeypatch.setenv("PSSBAM_REGION_GRID_SHIFT", str(shift))
    kern = getattr(pkg, f"KERNEL_{kernel}")
    for seed in rl.PSS_SEEDS:
        c = cases[seed]
        o = tl.PssOpts(region_len=n) if seed == rl.PSS_SEEDS[0] else tl.PssOpts(region_len=n, min_mq=10, up_ctx="CT", down_ctx="ACGTN")
        wf, wr, wst = oracle.pss(c.g, c.red, o)
        plain = finish(run(pkg, c, None, pss=pss_dict(o), kernel=kern))
        got = finish(run(pkg, c, c.ivs, regions_first=seed == rl.PSS_SEEDS[0], pss=pss_dict(o), kernel=kern))
        assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), (kernel, n, shift, seed)
        check_stats(got.stats, plain.stats, "pss_ok", "pss_filtered", int(wst[tl.ST_OK]))
        assert 0 < got.stats["pss_ok"] < plain.stats["pss_ok"]


def test_engine_overflow_path(pkg, oracle, cases, monkeypatch):
    """records longer than the staged prefix take the one-lane path and give the same tables"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    c = cases[rl.PSS_SEEDS[0]]
    for shift, n in ((4, 15), (10, 40)):
        monkeypatch.setenv("PSSBAM_REGION_GRID_SHIFT", str(shift))
        o = tl.PssOpts(region_len=n)
        wf, wr, wst = oracle.pss(c.g, c.red, o)
        got = finish(run(pkg, c, c.ivs, pss=pss_dict(o), kmer=dict(klen=4), kernel=pkg.KERNEL_TILED))
        assert got.stats["slow_path"] > 0
        assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), n
        k5, k3, kst = oracle.fragkon(c.g, c.red, tl.FkOpts(klen=4))
        assert np.array_equal(got.k5, k5.astype(np.uint64)) and np.array_equal(got.k3, k3.astype(np.uint64))
        assert got.stats["pss_ok"] == int(wst[tl.ST_OK]) and got.stats["kmer_ok"] == int(kst[tl.ST_OK])


# ---- composition: the filter picks no plane ------------------------------------------------------------------------

def sam_of(tmp_path, name, refs, recs):
    p = tmp_path / name
    tl.write_sam(p, refs, recs)
    return p


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_read_group_filter_and_read_groups(pkg, oracle, cases, monkeypatch, tmp_path, kernel, shift):
    """-T with -R, and with -G: each group's tables == the oracle on that group's reduced records"""
    monkeypatch.setenv("PSSBAM_REGION_GRID_SHIFT", str(shift))
    c = cases[rl.RG_SEEDS[0]]
    kern = getattr(pkg, f"KERNEL_{kernel}")
    ids = ["grpA", "grpB"]
    for n in (15, 40):
        o = tl.PssOpts(region_len=n, min_mq=3)
        want = {}
        for key in ids + [None]:
            sel = [r for r in c.kept if (first_rg(r) == key if key is not None else first_rg(r) not in ids)]
            want[key] = oracle.pss(c.g, sam_of(tmp_path, f"g{n}_{key}.sam", c.refs, sel), o)
        got = finish(run(pkg, c, c.ivs, pss=pss_dict(o), kernel=kern, read_group="grpA"))
        assert np.array_equal(got.fwd, want["grpA"][0]) and np.array_equal(got.rev, want["grpA"][1]), n
        assert got.stats["rg_dropped"] == sum(1 for r in c.recs if first_rg(r) != "grpA") and got.fwd.any()
        eng = run(pkg, c, c.ivs, pss=pss_dict(o), kernel=kern, read_groups=ids)
        planes = eng.finish_groups()
        eng.close()
        for key in ids + [None]:
            assert np.array_equal(planes[key].fwd, want[key][0]) and np.array_equal(planes[key].rev, want[key][1]), (n, key)
        assert planes["grpA"].fwd.any() and planes["grpB"].fwd.any()


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_length_bins_contig_sets_and_base_quality(pkg, oracle, cases, monkeypatch, tmp_path, kernel, shift):
    monkeypatch.setenv("PSSBAM_REGION_GRID_SHIFT", str(shift))
    c = cases[rl.PSS_SEEDS[1]]
    kern = getattr(pkg, f"KERNEL_{kernel}")
    edges = [30, 45, 70, 120]
    sets = {"big": ["chrB"], "rest": ["chrA", "scaffold_10", "notThere"]}
    masked = tmp_path / "masked.sam"
    bq.write_masked_sam(masked, c.refs, c.kept, 20)
    for n in (15, 40):
        o = tl.PssOpts(region_len=n, min_read_len=10)
        want = oracle_bins(oracle, c.g, c.red, o, edges)
        eng = run(pkg, c, c.ivs, pss=pss_dict(o), kernel=kern, length_bins=edges)
        got = eng.finish_bins()
        eng.close()
        assert list(got) == bins_of(o, edges)
        for key, (wf, wr) in want.items():
            assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), (n, key)
        assert sum(int(t.fwd.sum()) for t in got.values()) > 0
        want = oracle_sets(oracle, c.contigs, c.red, o, sets)
        eng = run(pkg, c, c.ivs, pss=pss_dict(o), kernel=kern, contig_sets=sets)
        got = eng.finish_sets()
        eng.close()
        for label, (wf, wr) in want.items():
            assert np.array_equal(got[label].fwd, wf) and np.array_equal(got[label].rev, wr), (n, label)
        assert got["big"].fwd.any() and got["rest"].fwd.any()
        wf, wr, _ = oracle.pss(c.g, masked, o)                                    # -Q 20
        got = finish(run(pkg, c, c.ivs, pss=pss_dict(o), kernel=kern, min_base_qual=20))
        assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), n
        eng = run(pkg, c, c.ivs, pss=pss_dict(o), kernel=kern, min_base_qual=20, length_bins=edges)   # -Q, -S and -T
        got = eng.finish_bins()
        eng.close()
        for key, (wf, wr) in oracle_bins(oracle, c.g, masked, o, edges).items():
            assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), (n, key)


def same_kmer(t, k5, k3):
    return np.array_equal(t.k5, k5.astype(np.uint64)) and np.array_equal(t.k3, k3.astype(np.uint64))


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_kmer_engine_and_its_planes(pkg, oracle, cases, monkeypatch, tmp_path, kernel, k, shift):
    """a k-mer engine: the totals, and each plane of -G / -S / -C, against the oracle on the plane's reduced records"""
    monkeypatch.setenv("PSSBAM_REGION_GRID_SHIFT", str(shift))
    kern = getattr(pkg, f"KERNEL_{kernel}")
    o = tl.FkOpts(klen=k, min_mq=5)
    fk = dict(klen=k, min_mq=5)
    c = cases[rl.FK_SEEDS[0]]
    k5, k3, kst = oracle.fragkon(c.g, c.red, o)
    plain = finish(run(pkg, c, None, kmer=fk, kernel=kern))
    got = finish(run(pkg, c, c.ivs, kmer=fk, kernel=kern))
    assert same_kmer(got, k5, k3) and k5.any() and k3.any()
    check_stats(got.stats, plain.stats, "kmer_ok", "kmer_filtered", int(kst[tl.ST_OK]))
    assert got.stats["kmer_fail"] == int(kst[tl.ST_KMER_FAIL])
    edges = [30, 45, 70]                                                          # -S: by strlen(SEQ)
    eng = run(pkg, c, c.ivs, kmer=fk, kernel=kern, length_bins=edges)
    planes = eng.finish_bins()
    eng.close()
    for lo, hi in zip([0] + edges, [e - 1 for e in edges] + [250000000]):
        w5, w3, _ = oracle.fragkon(c.g, c.red, tl.FkOpts(klen=k, min_mq=5, min_read_len=lo, max_read_len=hi))
        assert same_kmer(planes[(lo, hi)], w5, w3), (lo, hi)
    sets = {"big": ["chrB"], "rest": ["chrA", "scaffold_10", "notThere"]}          # -C
    eng = run(pkg, c, c.ivs, kmer=fk, kernel=kern, contig_sets=sets)
    planes = eng.finish_sets()
    eng.close()
    for label, names in sets.items():
        g = oracle.genome_from_arrays(tl.loaded_contigs([x for x in c.contigs if x[0] in names]))
        w5, w3, _ = oracle.fragkon(g, c.red, o)
        oracle.free_genome(g)
        assert same_kmer(planes[label], w5, w3), label
    c = cases[rl.RG_SEEDS[0]]                                                     # -G
    ids = ["grpA", "grpB"]
    eng = run(pkg, c, c.ivs, kmer=fk, kernel=kern, read_groups=ids)
    planes = eng.finish_groups()
    eng.close()
    for key in ids + [None]:
        sel = [r for r in c.kept if (first_rg(r) == key if key is not None else first_rg(r) not in ids)]
        w5, w3, _ = oracle.fragkon(c.g, sam_of(tmp_path, f"k_{key}.sam", c.refs, sel), o)
        assert same_kmer(planes[key], w5, w3), key
    assert planes["grpA"].k5.any()


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("k", [4, 8])
def test_combined_pss_and_kmer_engine(pkg, oracle, cases, monkeypatch, k, shift):
    monkeypatch.setenv("PSSBAM_REGION_GRID_SHIFT", str(shift))
    c = cases[rl.FK_SEEDS[0]]
    for n, kern in ((15, pkg.KERNEL_AUTO), (16, pkg.KERNEL_TILED), (40, pkg.KERNEL_AUTO), (15, pkg.KERNEL_SIMPLE)):
        o = tl.PssOpts(region_len=n)
        wf, wr, wst = oracle.pss(c.g, c.red, o)
        k5, k3, kst = oracle.fragkon(c.g, c.red, tl.FkOpts(klen=k))
        got = finish(run(pkg, c, c.ivs, pss=pss_dict(o), kmer=dict(klen=k), kernel=kern))
        assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr) and same_kmer(got, k5, k3), (n, kern)
        assert got.stats["pss_ok"] == int(wst[tl.ST_OK]) and got.stats["kmer_ok"] == int(kst[tl.ST_OK])


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("which", ["refid_64_and_up", "star_contig"])
def test_more_than_64_references(pkg, oracle, monkeypatch, tmp_path, which, shift):
    """ref_info and its region sibling leave the LDS cache: regions only on contigs with refID >= 64, and regions on a
    contig literally named "*" (the entry behind the last refID)"""
    monkeypatch.setenv("PSSBAM_REGION_GRID_SHIFT", str(shift))
    if which == "star_contig":
        contigs, refs, recs = _many_refs_dataset(rl.STAR_SEED)
        ivs = rl.STAR_IVS
    else:
        contigs, refs, recs = many_refs_dataset(rl.MANY_REFS_SEED, False)
        ivs = rl.MANY_REFS_IVS
    c = Case(oracle, tmp_path, which, contigs, refs, recs, ivs)
    try:
        for n, kern in ((20, pkg.KERNEL_TILED), (20, pkg.KERNEL_SIMPLE), (40, pkg.KERNEL_AUTO)):
            o = tl.PssOpts(region_len=n)
            wf, wr, wst = oracle.pss(c.g, c.red, o)
            k5, k3, _ = oracle.fragkon(c.g, c.red, tl.FkOpts(klen=4))
            got = finish(run(pkg, c, ivs, pss=pss_dict(o), kmer=dict(klen=4), kernel=kern))
            assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr) and same_kmer(got, k5, k3), (n, kern)
            assert got.stats["pss_ok"] == int(wst[tl.ST_OK]) > 0
        if which == "star_contig":   # the "*" records alone are tallied
            only = [iv for iv in ivs if iv[0] == "*"]
            wf, wr, _ = oracle.pss(c.g, sam_of(tmp_path, "star.sam", refs, rl.reduce_recs(recs, only)), tl.PssOpts(region_len=20))
            got = finish(run(pkg, c, only, pss=dict(region_len=20), kernel=pkg.KERNEL_TILED))
            assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr) and wf.any()
    finally:
        oracle.free_genome(c.g)


# ---- rules -----------------------------------------------------------------------------------------------------------

def test_rules(pkg, oracle, cases):
    E = pkg.PssbamError
    c = cases[rl.PSS_SEEDS[0]]
    o = tl.PssOpts(region_len=15)
    wf, wr, _ = oracle.pss(c.g, c.red, o)
    pf, pr, _ = oracle.pss(c.g, c.plain, o)
    names, name_of, starts, ends = rl.to_arrays(c.ivs)
    eng = pkg.Engine(pss=pss_dict(o))
    for bad in ((names, name_of, ends + 1, ends), (names, name_of + len(names), starts, ends), (names, -name_of - 1, starts, ends)):
        with pytest.raises(E) as ei:
            eng.set_regions(*bad)
        assert "error -1" in str(ei.value)                  # PSSBAM_EINVAL: start > end, name index out of range
    L = pkg.hip_lib()
    assert L.pssbam_engine_set_regions(eng._h, 1, None, 0, None, None, None) == -1
    assert L.pssbam_engine_set_regions(eng._h, 0, None, (1 << 26) + 1, None, None, None) == -1
    eng.set_regions(["chrB"], [0], [5], [5])                # only an empty interval: nothing is tallied
    eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
    eng.set_references([nm for nm, _ in c.refs])
    eng.submit(c.raw)
    got = eng.finish()
    assert not got.fwd.any() and not got.rev.any() and got.stats["pss_ok"] == 0 and got.stats["records"] == len(c.recs)
    eng.reset()
    eng.set_regions(names, name_of, starts, ends)           # legal again after reset, and after set_references
    eng.set_regions(names + names, np.concatenate([name_of, name_of + len(names)]), np.concatenate([starts, starts]),
                    np.concatenate([ends, ends]))           # a name given twice is the same contig
    eng.submit(c.raw)
    with pytest.raises(E) as ei:                            # records have been tallied
        eng.set_regions(names, name_of, starts, ends)
    assert "error -5" in str(ei.value)                      # PSSBAM_ESTATE
    first = eng.finish()
    assert np.array_equal(first.fwd, wf) and np.array_equal(first.rev, wr)
    eng.reset()                                             # the regions survive reset
    eng.submit(c.raw)
    again = eng.finish()
    assert np.array_equal(again.fwd, wf) and np.array_equal(again.rev, wr) and again.stats == first.stats
    eng.reset()
    eng.set_regions([], [], [], [])                         # no interval: off, the tables of an engine never given regions
    eng.submit(c.raw)
    off = eng.finish()
    eng.close()
    never = finish(run(pkg, c, None, pss=pss_dict(o)))
    assert np.array_equal(off.fwd, never.fwd) and np.array_equal(off.rev, never.rev) and off.stats == never.stats
    assert np.array_equal(off.fwd, pf) and np.array_equal(off.rev, pr)


def test_submit_bgzf_regions_set_after_feed_open(pkg, oracle, cases, tmp_path):
    c = cases[rl.PSS_SEEDS[1]]
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, c.refs, c.recs, rng=np.random.default_rng(3))
    for n in (15, 31):
        o = tl.PssOpts(region_len=n, min_mq=5)
        wf, wr, _ = oracle.pss(c.g, c.red, o)
        eng = pkg.Engine(pss=pss_dict(o))
        eng.feed_open(len(c.refs))
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        eng.set_regions(*rl.to_arrays(c.ivs))               # feeding has begun; set_references has not come
        eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
        eng.set_references([nm for nm, _ in c.refs])
        got = eng.finish()
        assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), n
        assert eng.feed_status()["flags"] == 0 and got.stats["records"] == len(c.recs)
        with pytest.raises(pkg.PssbamError):
            eng.set_regions(*rl.to_arrays(c.ivs))
        eng.close()


# ---- the command line ----------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    """a report file below its header lines (which echo the -F / -B / -o strings of the run)"""
    lines = text.splitlines(keepends=True)
    at = max(i for i, ln in enumerate(lines) if ln.startswith("### OUT:"))
    return "".join(lines[at + 1:])


def cli(exe, args, env, cwd):
    pr = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=300, cwd=cwd)
    assert pr.returncode == 0, pr.stderr
    return pr.stdout


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_T_matches_the_reduced_file(pkg, mode, tmp_path):
    """pss-bam -T and fragkon -T on the original file == the same binary without -T on the reduced file (and the
    reference on it), for the main tables and for every -S and -G plane file"""
    fmt, extra = CLI_MODES[mode]
    env = {**os.environ, **extra}
    contigs, refs, recs, ivs = rl.fuzz_case(rl.RG_SEEDS[0])
    recs = tl.ref_safe(recs, 4)
    hdr = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs) + "@RG\tID:grpA\tSM:a\n@RG\tID:grpB\tSM:b\n"
    tl.write_fasta(tmp_path / "g.fa", contigs)
    aln, red = f"in.{fmt}", f"red.{fmt}"
    write_aln(tmp_path / aln, fmt, refs, recs, hdr)
    write_aln(tmp_path / red, fmt, refs, rl.reduce_recs(recs, ivs), hdr)
    rl.write_bed(tmp_path / "t.bed", ivs)
    use_ref = tl.have_ref() and mode in ("bam_device_feed", "sam")
    pss, fk = pkg.PKG_DIR / "bin" / "pss-bam", pkg.PKG_DIR / "bin" / "fragkon"
    o = tl.PssOpts(region_len=31, min_mq=10, min_read_len=10)
    for sel in (["-S", "25,40,64"], ["-G"]):
        tag = sel[0][1]
        cli(pss, ["-F", "g.fa", "-B", aln, "-o", f"got{tag}", "-T", "t.bed"] + o.argv() + sel, env, tmp_path)
        cli(pss, ["-F", "g.fa", "-B", red, "-o", f"want{tag}"] + o.argv() + sel, env, tmp_path)
        cli(pss, ["-F", "g.fa", "-B", aln, "-o", f"plain{tag}"] + o.argv() + sel, env, tmp_path)
        files = sorted(p.name[len(f"want{tag}"):] for p in tmp_path.glob(f"want{tag}.*"))
        assert len(files) == (10 if tag == "S" else 6)                # -T writes no extra files, and leaves none out
        assert files == sorted(p.name[len(f"got{tag}"):] for p in tmp_path.glob(f"got{tag}.*"))
        for f in files:
            got = report_body((tmp_path / f"got{tag}{f}").read_text())
            assert got == report_body((tmp_path / f"want{tag}{f}").read_text()), f
        assert report_body((tmp_path / f"got{tag}.pss.counts.txt").read_text()) != report_body((tmp_path / f"plain{tag}.pss.counts.txt").read_text())
    if use_ref:
        _, _, wc, wr, _ = tl.run_ref_pss(tmp_path / "g.fa", tmp_path / red, tmp_path / "ref", o, bam2sam=str(pss.parent / "bam2sam"), timeout=300)
        assert report_body(wc) == report_body((tmp_path / "gotG.pss.counts.txt").read_text())
        assert report_body(wr) == report_body((tmp_path / "gotG.pss.rates.txt").read_text())
    ko = tl.FkOpts(klen=4, min_mq=5)
    for sel in (["-S", "25,40,64"], ["-G"]):
        tag = sel[0][1]
        got = cli(fk, ["-F", "g.fa", "-B", aln, "-T", "t.bed", "-o", f"kgot{tag}"] + ko.argv() + sel, env, tmp_path)
        want = cli(fk, ["-F", "g.fa", "-B", red, "-o", f"kwant{tag}"] + ko.argv() + sel, env, tmp_path)
        plain = cli(fk, ["-F", "g.fa", "-B", aln] + ko.argv(), env, tmp_path)
        assert table_of(got) == table_of(want) and table_of(got) != table_of(plain)
        files = sorted(p.name[len(f"kwant{tag}"):] for p in tmp_path.glob(f"kwant{tag}.*"))
        assert len(files) == (4 if tag == "S" else 2) and files == sorted(p.name[len(f"kgot{tag}"):] for p in tmp_path.glob(f"kgot{tag}.*"))
        for f in files:
            assert table_of((tmp_path / f"kgot{tag}{f}").read_text()) == table_of((tmp_path / f"kwant{tag}{f}").read_text()), f
    if use_ref:
        _, _, want, _ = tl.run_ref_fragkon(tmp_path / "g.fa", tmp_path / red, ko, bam2sam=str(fk.parent / "bam2sam"), timeout=300)
        assert table_of(want) == table_of(got)


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_cli_T_golden(pkg, fmt, tmp_path):
    """tests/golden/regions_setA.pss.{counts,rates}.txt are what the unmodified reference wrote for setA.sam reduced by
    tests/golden/regions_setA.bed, made in a scratch directory holding copies of setA.fa, setA.sam and the BED by

        Path("setA.regions.sam").write_text(regions_lib.reduce_sam_text(Path("setA.sam").read_text(), regions_lib.read_bed(Path("regions_setA.bed"))))
        pssbam_testlib.run_ref_pss(Path("setA.fa"), Path("setA.regions.sam"), Path("regions_setA"), pssbam_testlib.PssOpts())

    (oracle/_ref/pss-bam with its default options).  `pss-bam -T regions_setA.bed` on the whole setA must write the
    same tables."""
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(GOLD / "setA.fa"), "-B", str(GOLD / f"setA.{fmt}"), "-o", str(tmp_path / "out"),
                         "-T", str(GOLD / "regions_setA.bed")], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    for kind in ("counts", "rates"):
        want = report_body((GOLD / f"regions_setA.pss.{kind}.txt").read_text())
        assert report_body((tmp_path / f"out.pss.{kind}.txt").read_text()) == want, kind
        assert want != report_body((GOLD / f"pss_0.pss.{kind}.txt").read_text())

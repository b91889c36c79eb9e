"""pss-bam -Q on the GPU: read bases below a base quality are left out of the substitution tables.

The specification is one sentence: `-Q q` on a file == the tool without -Q on the same file with every SEQ base whose
quality is below q replaced by N.  So every check here runs the engine (or the command) with a minimum base quality on
the ORIGINAL records and compares with the CPU oracle (or the same binary, or the reference itself when oracle/_ref
exists) WITHOUT it on the masked copy that base_quality_lib writes (checked on its own in test_base_quality_host.py)."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import pssbam_testlib as tl
from test_gpu_contig_sets import oracle_sets
from test_gpu_length_bins import CLI_MODES, bins_of, oracle_bins, pss_dict
from test_gpu_read_groups import first_rg, rg_dataset

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
QS = [1, 20, 41, 42, 93]
NO_SLOW = ("slow_path",)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def run_engine(pkg, contigs, refs, raw, o: tl.PssOpts, kernel, q=0, **kw):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_group=o.read_group, min_base_qual=q, **kw)
    assert eng.min_base_qual == q
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(raw)
    return eng


def stats_but(st: dict, drop=NO_SLOW) -> dict:
    return {k: v for k, v in st.items() if k not in drop}


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    """the fuzz records (qualities uniform on 2..41, about 4 % without), their SAM, and one masked SAM per q"""
    contigs, refs, recs = tl.fuzz_dataset(9201, 3000)
    d = tmp_path_factory.mktemp("bq")
    sams = {0: d / "q0.sam"}
    tl.write_sam(sams[0], refs, recs)
    for q in QS:
        sams[q] = d / f"q{q}.sam"
        bq.write_masked_sam(sams[q], refs, recs, q)
    noq = d / "noqual.sam"
    tl.write_sam(noq, refs, [r for r in recs if r.qual == "*"])
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    yield contigs, refs, recs, sams, noq, g
    oracle.free_genome(g)


def test_the_comparison_is_not_vacuous(oracle, fuzz):
    """at q = 20 the masked and the unmasked oracle tables differ in interior cells of fwd and of rev"""
    contigs, refs, recs, sams, noq, g = fuzz
    for n in (15, 25, 31, 62):
        o = tl.PssOpts(region_len=n)
        pf, pr, _ = oracle.pss(g, sams[0], o)
        mf, mr, _ = oracle.pss(g, sams[20], o)
        assert (pf[2:] != mf[2:]).any() and (pr[2:] != mr[2:]).any()
        assert np.array_equal(pf[:2], mf[:2]) and np.array_equal(pr[:2], mr[:2])


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("n", [15, 25, 31, 62])
def test_engine_matches_oracle_on_masked_sam(pkg, oracle, fuzz, kernel, n):
    contigs, refs, recs, sams, noq, g = fuzz
    raw = tl.raw_records(refs, recs)
    rng = np.random.default_rng(300 + n)
    kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
    for trial in range(2):
        o = tl.random_pss_opts(rng) if trial else tl.PssOpts()
        o.region_len = n
        eng = run_engine(pkg, contigs, refs, raw, o, kern)
        plain = eng.finish()
        eng.close()
        eng = run_engine(pkg, contigs, refs, raw, o, kern, q=0)
        zero = eng.finish()
        eng.close()
        assert np.array_equal(zero.fwd, plain.fwd) and np.array_equal(zero.rev, plain.rev) and zero.stats == plain.stats
        for q in QS:
            wf, wr, _ = oracle.pss(g, sams[q], o)
            eng = run_engine(pkg, contigs, refs, raw, o, kern, q=q)
            got = eng.finish()
            eng.close()
            assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), (kernel, n, q, o)
            assert stats_but(got.stats) == stats_but(plain.stats), (kernel, n, q, o)
            assert np.array_equal(got.fwd[:2], plain.fwd[:2]) and np.array_equal(got.rev[:2], plain.rev[:2])
            if q >= 42:   # every quality there is lies below: only the records without qualities are left
                nf, nr, _ = oracle.pss(g, noq, o)
                assert np.array_equal(got.fwd[2:], nf[2:]) and np.array_equal(got.rev[2:], nr[2:])


def test_engine_overflow_path(pkg, oracle, fuzz, monkeypatch):
    """records longer than the staged prefix take the one-lane path and give the same tables"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    contigs, refs, recs, sams, noq, g = fuzz
    raw = tl.raw_records(refs, recs)
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        for q in (20, 41):
            wf, wr, _ = oracle.pss(g, sams[q], o)
            eng = run_engine(pkg, contigs, refs, raw, o, pkg.KERNEL_TILED, q=q)
            got = eng.finish()
            eng.close()
            assert got.stats["slow_path"] > 0
            assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), (n, q)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_read_group_filter(pkg, oracle, kernel, tmp_path):
    """-Q with -R"""
    contigs, refs, recs = tl.fuzz_dataset(9202, 3000, with_rg=True)
    keep = [r for r in recs if first_rg(r) == "grpA"]
    sam = tmp_path / "keep.sam"
    bq.write_masked_sam(sam, refs, keep, 20)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
        for n in (15, 31):
            o = tl.PssOpts(region_len=n, min_mq=3)
            wf, wr, _ = oracle.pss(g, sam, o)
            eng = run_engine(pkg, contigs, refs, tl.raw_records(refs, recs), tl.PssOpts(**{**pss_dict(o), "read_group": "grpA"}), kern, q=20)
            got = eng.finish()
            eng.close()
            assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), n
            assert got.stats["rg_dropped"] == len(recs) - len(keep)
    finally:
        oracle.free_genome(g)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_read_groups(pkg, oracle, kernel, tmp_path):
    """-Q with -G: each group's tables == the oracle on that group's masked records"""
    ids = ["grpA", "grpB", "lib 3"]
    contigs, refs, recs = rg_dataset(9203, ids)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
        for n in (15, 40):
            o = tl.PssOpts(region_len=n)
            eng = run_engine(pkg, contigs, refs, tl.raw_records(refs, recs), o, kern, q=20, read_groups=ids)
            got = eng.finish_groups()
            eng.close()
            for key in ids + [None]:
                sel = [r for r in recs if (first_rg(r) == key if key is not None else first_rg(r) not in ids)]
                sam = tmp_path / f"g{n}_{ids.index(key) if key else 'none'}.sam"
                bq.write_masked_sam(sam, refs, sel, 20)
                wf, wr, _ = oracle.pss(g, sam, o)
                assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), (n, key)
    finally:
        oracle.free_genome(g)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_length_bins(pkg, oracle, fuzz, kernel):
    """-Q with -S, 4 edges"""
    contigs, refs, recs, sams, noq, g = fuzz
    kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
    edges = [30, 45, 70, 120]
    for n in (15, 40):
        o = tl.PssOpts(region_len=n, min_read_len=10)
        want = oracle_bins(oracle, g, sams[20], o, edges)
        eng = run_engine(pkg, contigs, refs, tl.raw_records(refs, recs), o, kern, q=20, length_bins=edges)
        got = eng.finish_bins()
        eng.close()
        assert list(got) == bins_of(o, edges)
        for key, (wf, wr) in want.items():
            assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), (n, key)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_contig_sets(pkg, oracle, fuzz, kernel):
    """-Q with -C"""
    contigs, refs, recs, sams, noq, g = fuzz
    kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
    sets = {"big": ["chrB"], "rest": ["chrA", "scaffold_10", "notThere"]}
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        want = oracle_sets(oracle, contigs, sams[20], o, sets)
        eng = run_engine(pkg, contigs, refs, tl.raw_records(refs, recs), o, kern, q=20, contig_sets=sets)
        got = eng.finish_sets()
        eng.close()
        for label, (wf, wr) in want.items():
            assert np.array_equal(got[label].fwd, wf) and np.array_equal(got[label].rev, wr), (n, label)


@pytest.mark.parametrize("klen", [4, 7])
def test_with_kmer_tally_in_the_same_engine(pkg, oracle, fuzz, klen):
    """a PSS + k-mer engine: the substitution tables are masked, the k-mer tables are those of the unmasked run"""
    contigs, refs, recs, sams, noq, g = fuzz
    raw = tl.raw_records(refs, recs)
    for n in (15, 31):
        o = tl.PssOpts(region_len=n)
        res = {}
        for q in (0, 20):
            eng = pkg.Engine(pss=pss_dict(o), kmer=dict(klen=klen), min_base_qual=q)
            eng.set_genome_arrays(tl.loaded_contigs(contigs))
            eng.set_references([nm for nm, _ in refs])
            eng.submit(raw)
            res[q] = eng.finish()
            eng.close()
        wf, wr, _ = oracle.pss(g, sams[20], o)
        assert np.array_equal(res[20].fwd, wf) and np.array_equal(res[20].rev, wr)
        assert np.array_equal(res[20].k5, res[0].k5) and np.array_equal(res[20].k3, res[0].k3)
        assert res[0].k5.any() and stats_but(res[20].stats) == stats_but(res[0].stats)


def test_rules(pkg, oracle, fuzz):
    E = pkg.PssbamError
    contigs, refs, recs, sams, noq, g = fuzz
    for bad in (-1, 94, 255, 1 << 20):
        with pytest.raises(E):
            pkg.Engine(pss=dict(region_len=5), min_base_qual=bad)
    with pytest.raises(E):                                  # nothing to mask on a k-mer engine
        pkg.Engine(kmer=dict(klen=4), min_base_qual=20)
    eng = pkg.Engine(kmer=dict(klen=4))
    with pytest.raises(E) as ei:
        eng.set_min_base_quality(0)
    assert "error -1" in str(ei.value)                      # PSSBAM_EINVAL
    eng.close()
    o = tl.PssOpts(region_len=15)
    eng = pkg.Engine(pss=pss_dict(o))
    for bad in (-1, 94):
        with pytest.raises(E) as ei:
            eng.set_min_base_quality(bad)
        assert "error -1" in str(ei.value)
    assert eng.min_base_qual == 0
    eng.set_min_base_quality(93)
    eng.set_min_base_quality(20)                            # may be changed until the first tally
    assert eng.min_base_qual == 20
    raw = tl.raw_records(refs, recs)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(raw)
    with pytest.raises(E) as ei:                            # records have been tallied
        eng.set_min_base_quality(30)
    assert "error -5" in str(ei.value)                      # PSSBAM_ESTATE
    assert eng.min_base_qual == 20
    wf, wr, _ = oracle.pss(g, sams[20], o)
    first = eng.finish()
    assert np.array_equal(first.fwd, wf) and np.array_equal(first.rev, wr)
    eng.reset()                                             # the value survives reset
    eng.submit(raw)
    again = eng.finish()
    assert np.array_equal(again.fwd, wf) and np.array_equal(again.rev, wr)
    eng.reset()
    eng.set_min_base_quality(41)                            # legal again after reset
    eng.submit(raw)
    wf, wr, _ = oracle.pss(g, sams[41], o)
    got = eng.finish()
    assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr)
    eng.reset()
    eng.set_min_base_quality(0)                             # and off again: the plain tables
    eng.submit(raw)
    wf, wr, _ = oracle.pss(g, sams[0], o)
    got = eng.finish()
    assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr)
    eng.close()


def test_submit_bgzf_quality_set_after_feed_open(pkg, oracle, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(9204, 4000)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    sam = tmp_path / "masked.sam"
    bq.write_masked_sam(sam, refs, recs, 20)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        for n in (15, 31):
            o = tl.PssOpts(region_len=n, min_mq=5)
            wf, wr, _ = oracle.pss(g, sam, o)
            eng = pkg.Engine(pss=pss_dict(o))
            eng.feed_open(len(refs))
            eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
            eng.set_min_base_quality(20)
            eng.set_genome_arrays(tl.loaded_contigs(contigs))
            eng.set_references([nm for nm, _ in refs])
            got = eng.finish()
            assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr), n
            assert eng.feed_status()["flags"] == 0 and got.stats["records"] == len(recs)
            with pytest.raises(pkg.PssbamError):
                eng.set_min_base_quality(21)
            eng.close()
    finally:
        oracle.free_genome(g)


# ---- the command line ----------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    """a report file below its header lines (which echo the -F / -B / -o strings of the run)"""
    lines = text.splitlines(keepends=True)
    at = max(i for i, ln in enumerate(lines) if ln.startswith("### OUT:"))
    return "".join(lines[at + 1:])


@pytest.mark.parametrize("mode", list(CLI_MODES))
@pytest.mark.parametrize("n", [15, 31])
def test_cli_Q_matches_the_masked_file(pkg, mode, n, tmp_path):
    """pss-bam -Q 20 on the original file == the same binary without -Q on the masked file (and the reference on it)"""
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    contigs, refs, recs = tl.fuzz_dataset(9205, 6000)
    recs = tl.ref_safe(recs)
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, contigs)
    aln, masked = tmp_path / f"in.{fmt}", tmp_path / f"masked.{fmt}"
    if fmt == "bam":
        tl.write_bam(aln, refs, recs, rng=np.random.default_rng(2))
        tl.write_bam(masked, refs, bq.mask_recs(recs, 20), rng=np.random.default_rng(2))
    else:
        tl.write_sam(aln, refs, recs)
        bq.write_masked_sam(masked, refs, recs, 20)
    o = tl.PssOpts(region_len=n, min_mq=10, min_read_len=10)
    env = {**os.environ, **extra}
    got_p, want_p, plain_p = tmp_path / "got", tmp_path / "want", tmp_path / "plain"
    pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(got_p), "-Q", "20"] + o.argv(), capture_output=True,
                        text=True, env=env, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(" -Q 20")
    pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(masked), "-o", str(want_p)] + o.argv(), capture_output=True,
                        text=True, env=env, timeout=300)
    assert pr.returncode == 0, pr.stderr
    pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(plain_p), "-Q", "0"] + o.argv(), capture_output=True,
                        text=True, env=env, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert sorted(p.name for p in tmp_path.glob("*.txt")) == sorted(f"{p}.pss.{k}.txt" for p in ("got", "want", "plain")
                                                                     for k in ("counts", "rates"))
    for kind in ("counts", "rates"):
        got = report_body(Path(f"{got_p}.pss.{kind}.txt").read_text())
        assert got == report_body(Path(f"{want_p}.pss.{kind}.txt").read_text()), kind
        assert got != report_body(Path(f"{plain_p}.pss.{kind}.txt").read_text()), kind     # -Q 0: the unmasked tables
    if tl.have_ref() and mode in ("bam_device_feed", "sam"):
        _, _, wc, wr, _ = tl.run_ref_pss(fa, masked, tmp_path / "ref", o, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
        assert report_body(wc) == report_body(Path(f"{got_p}.pss.counts.txt").read_text())
        assert report_body(wr) == report_body(Path(f"{got_p}.pss.rates.txt").read_text())


@pytest.mark.parametrize("fmt", ["bam", "sam"])
def test_cli_Q_golden(pkg, fmt, tmp_path):
    """tests/golden/bq20_setA.pss.{counts,rates}.txt are what the unmodified reference wrote for setA.sam masked at
    q = 20, made in a scratch directory holding copies of setA.fa and setA.sam by

        Path("setA.bq20.sam").write_text(base_quality_lib.mask_sam_text(Path("setA.sam").read_text(), 20))
        pssbam_testlib.run_ref_pss(Path("setA.fa"), Path("setA.bq20.sam"), Path("bq20_setA"), pssbam_testlib.PssOpts())

    (oracle/_ref/pss-bam with its default options).  `pss-bam -Q 20` on the unmasked setA must write the same tables."""
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(GOLD / "setA.fa"), "-B", str(GOLD / f"setA.{fmt}"), "-o", str(tmp_path / "out"), "-Q", "20"],
                        capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    for kind in ("counts", "rates"):
        want = report_body((GOLD / f"bq20_setA.pss.{kind}.txt").read_text())
        assert report_body((tmp_path / f"out.pss.{kind}.txt").read_text()) == want, kind

"""pss-bam -I on the GPU: clipped and gapped reads tallied by their anchored ends.

The specification is gapped_lib's: the engine (or the command) with the setting on the ORIGINAL records == the tool
without it on the records in which every anchoring record has been replaced by its <span>M record.  So every check
here compares with the CPU oracle (or the reference itself where oracle/_ref exists) on the anchored copies, which
test_gapped_host.py checks against a direct count on the CPU."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import gapped_lib as gl
import pssbam_testlib as tl
import regions_lib as rl
from test_gapped_host import N_RECS, SEEDS
from test_gpu_length_hist import CLI_MODES, pss_dict, write_aln

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def kern_of(pkg, kernel):
    return pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, gapped=True, **kw):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_group=o.read_group, gapped=gapped, **kw)
    assert eng.gapped is gapped
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if len(recs):
        eng.submit(tl.raw_records(refs, recs))
    return eng


def tables_of(pkg, contigs, refs, recs, o, kernel, gapped=True, **kw):
    eng = run_engine(pkg, contigs, refs, recs, o, kernel, gapped, **kw)
    got = eng.finish()
    eng.close()
    return got


def stats_but(st: dict) -> dict:
    return {k: v for k, v in st.items() if k != "slow_path"}


def same(got, want, ctx=""):
    assert np.array_equal(got.fwd, want[0]) and np.array_equal(got.rev, want[1]), ctx


def oracle_on(oracle, tmp_path, contigs, refs, recs, o, tag="x"):
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        sam = tmp_path / f"{tag}.sam"
        tl.write_sam(sam, refs, recs)
        return oracle.pss(g, sam, o)[:2]
    finally:
        oracle.free_genome(g)


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    contigs, refs, recs, _ = gl.fuzz_case(SEEDS[0], N_RECS)
    anchored = gl.anchor_recs(recs)
    sam = tmp_path_factory.mktemp("gapped") / "anchored.sam"
    tl.write_sam(sam, refs, anchored)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    yield contigs, refs, recs, anchored, sam, g
    oracle.free_genome(g)


# ---- parity ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("n", [15, 25, 31, 40, 62])
def test_engine_matches_oracle_on_anchored_sam(pkg, oracle, fuzz, kernel, n):
    """one, two and three row passes; a count read through the wrong anchor, a blanking edge off by one or a count in the
    wrong pass shows here"""
    contigs, refs, recs, anchored, sam, g = fuzz
    rng = np.random.default_rng(600 + n)
    kern = kern_of(pkg, kernel)
    for trial in range(3):
        o = tl.random_pss_opts(rng) if trial else tl.PssOpts()
        o.region_len = n
        want = oracle.pss(g, sam, o)[:2]
        got = tables_of(pkg, contigs, refs, recs, o, kern)
        same(got, want, (kernel, n, o))
        twin = tables_of(pkg, contigs, refs, anchored, o, kern, gapped=False)       # the engine without the setting on the anchored records
        same(got, (twin.fwd, twin.rev), (kernel, n, o))
        assert stats_but(got.stats) == stats_but(twin.stats), (kernel, n, o)
        if not trial:
            plain = tables_of(pkg, contigs, refs, recs, o, kern, gapped=False)
            assert plain.stats["slow_path"] == 0
            # more than 200 reads' worth: an unpaired read adds one count per row to either table
            assert int(got.fwd.sum() + got.rev.sum()) - int(plain.fwd.sum() + plain.rev.sum()) > 200 * 2 * (n + 2) * 3 // 4, (kernel, n)
            assert got.stats["pss_ok"] > plain.stats["pss_ok"] + 200


# ---- one indel at every distance from either end: every expected row sum is known by hand -------------------------------

HAND_SPAN = 200


def hand_case(n: int, guard: bool):
    """Reads that copy a random A/C/G/T contig over HAND_SPAN reference bases, each with one 3-base deletion or one 2-base
    insertion at distance d = 1 .. n + 1 from the left or from the right end of the alignment, on both strands.  With
    `guard` a second deletion sits in the middle, further than n from both ends, so the run at the far end of the probe
    begins outside the probed end's window: that end counts row 2 + i exactly when its run is longer than i (d > i).
    Without it the positions behind the probe are read through the other end's anchor: behind a deletion of 3 every row
    counts but the three deleted positions, behind an insertion every row.  The other end always counts every row.
    -> (contigs, refs, recs, expected row sums of rows 2.. of (fwd, rev))"""
    rng = np.random.default_rng(1234 + n)
    ctg = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=1500))
    recs = []
    rows = [np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)]
    for is_rev in (False, True):
        for kind in ("D", "I"):
            for from_left in (True, False):
                for d in range(1, n + 2):
                    s = 10 + 3 * len(recs) % 1000
                    # alignment columns left to right as (op, length); the probe is d columns from its end
                    rest = HAND_SPAN - d - (3 if kind == "D" else 0)
                    ops = [(d, "M"), (3, "D") if kind == "D" else (2, "I")]
                    ops += [(rest // 2, "M"), (4, "D"), (rest - rest // 2 - 4, "M")] if guard else [(rest, "M")]
                    if not from_left:
                        ops = ops[::-1]
                    seq, p = [], s
                    for ln, op in ops:
                        if op == "M":
                            seq.append(ctg[p:p + ln])
                            p += ln
                        elif op == "D":
                            p += ln
                        else:
                            seq.append("".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=ln)))
                    assert p - s == HAND_SPAN
                    seq = "".join(seq)
                    recs.append(tl.Rec(f"h{len(recs):04d}", 16 if is_rev else 0, "hand", s + 1, 30, ops, seq=seq, qual="I" * len(seq)))
                    probed = np.array([i < d or (not guard and (kind == "I" or i >= d + 3)) for i in range(n)], dtype=np.int64)
                    full = np.ones(n, dtype=np.int64)
                    left_rows, right_rows = (probed, full) if from_left else (full, probed)
                    # forward read: left end -> fwd table, right end -> rev table; reverse-strand read: the other way round
                    rows[1 if is_rev else 0] += left_rows
                    rows[0 if is_rev else 1] += right_rows
    return [("hand", ctg)], [("hand", len(ctg))], recs, rows


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("guard", [True, False])
@pytest.mark.parametrize("n", [30, 40])
def test_indel_at_every_distance(pkg, kernel, n, guard):
    """pins the right-end anchor and the blanking edge at every offset, rows 31 | 32 included (guard: in the tiled kernel's
    lanes, slow_path stays 0), and the positions read through the other end's anchor (no guard)"""
    contigs, refs, recs, rows = hand_case(n, guard)
    got = tables_of(pkg, contigs, refs, recs, tl.PssOpts(region_len=n), kern_of(pkg, kernel))
    assert got.stats["pss_ok"] == len(recs) == 8 * (n + 1)
    if guard and kernel == "TILED":
        assert got.stats["slow_path"] == 0
    for t, want in ((got.fwd, rows[0]), (got.rev, rows[1])):
        off = t[2:].copy()
        off[:, [0, 5, 10, 15]] = 0
        assert not off.any(), (kernel, n, guard, np.argwhere(off)[:8])              # (the mirror of a diagonal cell is a diagonal cell)
        assert np.array_equal(t[2:].sum(axis=1).astype(np.int64), want), (kernel, n, guard)
        assert np.array_equal(t[:2].sum(axis=1), [len(recs), len(recs)])


# ---- the op cap, the one-lane path ------------------------------------------------------------------------------------------

def capped_rec(contig: str, n_ops: int, s: int) -> tl.Rec:
    """a read copying `contig` from s (or the next start whose two context bases are A/C/G/T) with n_ops CIGAR ops: 90
    matched bases at either end, the gaps in between"""
    k = (n_ops - 1) // 2
    ops = [(7, "S")] if n_ops % 2 == 0 else []
    ops.append((90, "M"))
    for t in range(k):
        ops.append((1 + t % 3, "ID"[t & 1]))
        ops.append((90 if t == k - 1 else 5, "M"))
    assert len(ops) == n_ops
    span = sum(ln for ln, op in ops if op in "MD")
    while contig[s - 1].upper() not in "ACGT" or contig[s + span].upper() not in "ACGT":
        s += 1
    seq, p = [], s
    for ln, op in ops:
        if op in "SI":
            seq.append("ACGT"[ln & 3] * ln)
        elif op == "M":
            seq.append(contig[p:p + ln].upper())
            p += ln
        else:
            p += ln
    seq = "".join(seq)
    return tl.Rec(f"cap{n_ops}", 0, "chrB", s + 1, 40, ops, seq=seq, qual="F" * len(seq))


def test_op_cap(pkg, oracle, fuzz, tmp_path):
    contigs, refs = fuzz[0], fuzz[1]
    cap = pkg.GAPPED_TILED_OPS
    o = tl.PssOpts(region_len=30)
    for n_ops, slow in ((cap - 1, 0), (cap, 0), (cap + 1, 1)):
        rec = capped_rec(dict(contigs)["chrB"], n_ops, 1000 + 7 * n_ops)
        assert gl.anchor_info(rec) is not None and len(rec.cigar) == n_ops
        want = oracle_on(oracle, tmp_path, contigs, refs, [gl.anchor_rec(rec)], o, f"cap{n_ops}")
        got = tables_of(pkg, contigs, refs, [rec], o, pkg.KERNEL_TILED)
        same(got, want, n_ops)
        assert got.stats["slow_path"] == slow and got.stats["pss_ok"] == 1 and int(got.fwd.sum()) > 25, (n_ops, got.stats)


def test_overflow_path(pkg, oracle, fuzz, monkeypatch):
    """records longer than the staged prefix take the one-lane path and give the same tables"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    contigs, refs, recs, anchored, sam, g = fuzz
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        got = tables_of(pkg, contigs, refs, recs, o, pkg.KERNEL_TILED)
        assert got.stats["slow_path"] > 0
        same(got, oracle.pss(g, sam, o)[:2], n)


# ---- compositions ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_read_group_filter(pkg, oracle, kernel, tmp_path):
    contigs, refs, recs, _ = gl.fuzz_case(9503, N_RECS, with_rg=True)
    keep = [r for r in gl.anchor_recs(recs) if ("RG", "Z", "grpA") in r.tags]
    for n in (15, 40):
        o = tl.PssOpts(region_len=n, min_mq=3)
        want = oracle_on(oracle, tmp_path, contigs, refs, keep, o, f"rg{n}")
        got = tables_of(pkg, contigs, refs, recs, tl.PssOpts(**{**pss_dict(o), "read_group": "grpA"}), kern_of(pkg, kernel))
        assert got.stats["rg_dropped"] == len(recs) - len(keep) and int(got.fwd[2:].sum()) > 1000
        same(got, want, (kernel, n))


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_min_base_quality(pkg, oracle, fuzz, kernel, tmp_path):
    """the anchored record's filler carries quality 0: masked like every base below the threshold"""
    contigs, refs, recs, anchored, sam, g = fuzz
    low = bq.mask_recs(anchored, 20)
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        want = oracle_on(oracle, tmp_path, contigs, refs, low, o, f"q{n}")
        got = tables_of(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), min_base_qual=20)
        same(got, want, (kernel, n))
        unmasked = oracle.pss(g, sam, o)[0]
        assert (got.fwd[2:] != unmasked[2:]).any() and int(got.fwd[2:].sum()) > 1000


def deleted_stretches(recs, names) -> list:
    """[(contig, start, end)] of the reference bases under the first D op of the anchoring records"""
    out = []
    for r in recs:
        if gl.anchor_info(r) is None or r.rname not in names or r.pos < 1:
            continue
        p = r.pos - 1
        for ln, op in r.cigar:
            if op == "D":
                out.append((r.rname, p, p + ln))
                break
            if op in "M=X":
                p += ln
    return out


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_regions(pkg, oracle, fuzz, kernel, tmp_path):
    """-T sees the alignment [s, s + span): also an interval that only a read's deleted stretch overlaps keeps the read"""
    contigs, refs, recs, anchored, sam, g = fuzz
    ivs = rl.fuzz_intervals(SEEDS[0], contigs, recs)
    dels = deleted_stretches(recs, {"scaffold_10"})          # fuzz_intervals puts nothing on this contig
    assert len(dels) >= 5
    ivs += [(nm, a, a + 1) for nm, a, _ in dels[:5]]
    kept = rl.reduce_recs(anchored, ivs)
    assert 50 < len(kept) < len(recs) - 50 and any(r.rname == "scaffold_10" for r in kept)
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        want = oracle_on(oracle, tmp_path, contigs, refs, kept, o, f"t{n}")
        eng = run_engine(pkg, contigs, refs, [], o, kern_of(pkg, kernel))
        eng.set_regions(*rl.to_arrays(ivs))
        eng.submit(tl.raw_records(refs, recs))
        got = eng.finish()
        eng.close()
        same(got, want, (kernel, n))
        assert int(got.fwd[2:].sum()) > 300


# ---- rules -------------------------------------------------------------------------------------------------------------------

def test_rules(pkg, oracle, fuzz, tmp_path):
    E = pkg.PssbamError
    for cfg in (dict(kmer=dict(klen=4)), dict(pss=dict(region_len=5), kmer=dict(klen=4))):
        with pytest.raises(E):                              # PSSBAM_TALLY_KMER in the mask
            pkg.Engine(gapped=True, **cfg)
    for other in (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]}), dict(length_hist=100),
                  dict(site_context="cpg"), dict(end_condition=(1, 13, 13))):
        eng = pkg.Engine(pss=dict(region_len=5), **other)
        with pytest.raises(E):                              # planes, -H, -X or -E set: no gapped reads
            eng.set_gapped(True)
        assert eng.gapped is False
        eng.set_gapped(False)                               # off stays legal
        eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), gapped=True)
    n_words = eng.counters_device()[1]
    assert n_words == eng.counter_layout()["n_u64"] == 2 * 7 * 16 + pkg.ST_N     # no counter words, no stats slot
    for setter, arg in ((eng.set_read_groups, ["a"]), (eng.set_length_bins, [30]), (eng.set_contig_sets, {"x": ["chrA"]}),
                        (eng.set_length_histogram, 100), (eng.set_site_context, "cpg")):
        with pytest.raises(E):                              # and the other way round
            setter(arg)
    with pytest.raises(E):
        eng.set_end_condition(1, 13, 13)
    assert eng.gapped and eng.read_groups == [] and eng.length_bins == [] and eng.contig_sets == [] and eng.length_hist == 0
    assert eng.site_context is None and eng.end_condition is None and eng.counters_device()[1] == n_words
    eng.set_gapped(False)                                   # off again: the others are legal
    eng.set_length_histogram(100)
    eng.close()

    contigs, refs, recs, anchored, sam, g = fuzz
    o = tl.PssOpts(region_len=15)
    want = oracle.pss(g, sam, o)[:2]
    plain_want = oracle_on(oracle, tmp_path, contigs, refs, recs, o, "plain")
    eng, owner = pkg.Engine(pss=pss_dict(o), gapped=True, min_base_qual=0), pkg.Engine(pss=pss_dict(o))
    d, nw = owner.counters_device()
    owner.sync()
    eng.bind_counters(d, nw)                                # a bound block is fine: the block does not change size
    eng.set_gapped(False)
    eng.set_gapped(True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    for on in (False, True):
        with pytest.raises(E):                              # records have been tallied
            eng.set_gapped(on)
    same(eng.finish(), want)
    eng.reset()                                             # the setting survives reset
    assert eng.gapped
    eng.submit(tl.raw_records(refs, recs))
    same(eng.finish(), want)
    eng.reset()
    eng.set_gapped(False)                                   # legal again after reset
    eng.submit(tl.raw_records(refs, recs))
    same(eng.finish(), plain_want)
    eng.close()
    owner.close()


def test_submit_bgzf_setting_after_feed_open(pkg, oracle, fuzz, tmp_path):
    contigs, refs, recs, anchored, sam, g = fuzz
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    o = tl.PssOpts(region_len=25, min_mq=5)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_gapped(True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    got = eng.finish()
    assert eng.feed_status()["flags"] == 0 and got.stats["records"] == len(recs)
    same(got, oracle.pss(g, sam, o)[:2])
    eng.close()


# ---- the command line ------------------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    """a report without its three path lines"""
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_I(pkg, oracle, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    contigs, refs, recs, _ = gl.fuzz_case(9504, 6000)
    recs = tl.ref_safe(recs)
    anchored = gl.anchor_recs(recs)
    assert tl.ref_safe(anchored) == anchored
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, contigs)
    aln, anc = tmp_path / f"in.{fmt}", tmp_path / f"anchored.{fmt}"
    write_aln(aln, fmt, refs, recs)
    write_aln(anc, fmt, refs, anchored)
    o = tl.PssOpts(region_len=25, min_mq=10)
    env = {**os.environ, **extra}

    def run(aln_path, out, *more):
        pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln_path), "-o", str(tmp_path / out), *more] + o.argv(), capture_output=True,
                            text=True, env=env, timeout=300)
        assert pr.returncode == 0, pr.stderr
        return pr.stderr, Path(f"{tmp_path / out}.pss.counts.txt").read_text(), Path(f"{tmp_path / out}.pss.rates.txt").read_text()

    err, counts, rates = run(aln, "out", "-I")
    assert err.splitlines()[0].endswith(" -I")
    assert sorted(p.name for p in tmp_path.glob("out.*")) == ["out.pss.counts.txt", "out.pss.rates.txt"]
    want = oracle_on(oracle, tmp_path, contigs, refs, anchored, o, "want")
    got = tl.parse_counts_text(counts)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    # the same binary without -I: on the anchored file the same reports, on the original file the plain tables
    err2, counts2, rates2 = run(anc, "twin")
    assert not err2.splitlines()[0].endswith(" -I")
    assert report_body(counts2) == report_body(counts) and report_body(rates2) == report_body(rates)
    _, counts3, _ = run(aln, "plain")
    plain = oracle_on(oracle, tmp_path, contigs, refs, recs, o, "plainwant")
    got3 = tl.parse_counts_text(counts3)
    assert np.array_equal(got3[0], plain[0]) and np.array_equal(got3[1], plain[1]) and int(got[0].sum()) > int(got3[0].sum()) + 2000
    if tl.have_ref() and mode in ("bam_device_feed", "sam"):
        _, _, wc, wr, _ = tl.run_ref_pss(fa, anc, tmp_path / "ref", o, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
        assert report_body(wc) == report_body(counts) and report_body(wr) == report_body(rates)

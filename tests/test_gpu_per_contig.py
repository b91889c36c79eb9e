"""pss-bam -A on the GPU: every BAM reference's own pair of substitution tables in one pass over the records.  Plane k
must equal what the reference computes with a FASTA that holds only contig k (the CPU oracle on the reduced genome; for
the command line also -C with one set per contig from the same binary, and the reference itself when oracle/_ref
exists); the planes must sum to the totals, the totals and the status counters must equal a run without the setting,
and a reference that holds nothing must not show up."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import pssbam_testlib as tl
import regions_lib as rl

pytestmark = pytest.mark.gpu

KERNELS = {"AUTO": 0, "SIMPLE": 1, "TILED": 2}
LENS = (5000, 1200, 300, 900, 700)   # five contigs: more than one or two LDS slots hold


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq,
                up_ctx=o.up_ctx, down_ctx=o.down_ctx, merged_only=o.merged_only)


def oracle_planes(oracle, contigs, refs, sam: Path, o: tl.PssOpts) -> dict:
    """{plane: (fwd, rev)} of the oracle on the genome reduced to the plane's contig, for the planes that hold
    something: plane k = header name k, plane len(refs) = the contig named "*" (the refID -1 records)"""
    out = {}
    for k, nm in enumerate([nm for nm, _ in refs] + ["*"]):
        keep = [c for c in contigs if c[0] == nm]
        if not keep or (nm == "*" and k < len(refs)):   # (a header name "*" would be written as refID -1)
            continue
        g = oracle.genome_from_arrays(tl.loaded_contigs(keep))
        try:
            f, r, _ = oracle.pss(g, sam, o)
        finally:
            oracle.free_genome(g)
        if f.any() or r.any():
            out[k] = (f, r)
    return out


def make_engine(pkg, contigs, refs, o: tl.PssOpts, kernel, per_contig=True, **kw):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_group=o.read_group, per_contig=per_contig, **kw)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    return eng


def plane(eng, k):
    fwd = np.ones((eng.region_len + 2, 16), dtype=np.uint64)
    rev = np.ones_like(fwd)
    assert eng._L.pssbam_engine_finish_groups(eng._h, k, fwd.ctypes.data, rev.ctypes.data) == 0
    return fwd, rev


def check_engine(eng, want: dict, n_ref: int):
    """planes == want (and no other plane is touched), planes sum to the totals, the leading pair is zero"""
    got = eng.finish_contigs()
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for k, (wf, wr) in want.items():
        assert np.array_equal(got[k].fwd, wf) and np.array_equal(got[k].rev, wr), k
    tot = eng.finish()
    rows = eng.region_len + 2
    zero = np.zeros((rows, 16), dtype=np.uint64)
    assert np.array_equal(sum((t.fwd for t in got.values()), zero), tot.fwd)
    assert np.array_equal(sum((t.rev for t in got.values()), zero), tot.rev)
    p0f, p0r = plane(eng, -1)
    assert not p0f.any() and not p0r.any()
    for k in (0, n_ref, max(want, default=0)):   # finish_groups(k) is plane k, touched or not
        f, r = plane(eng, k)
        assert np.array_equal(f, want[k][0] if k in want else zero) and np.array_equal(r, want[k][1] if k in want else zero)
    lay = eng.counter_layout()
    assert lay["n_u64"] == eng.counters_device()[1] and lay["contigs"]["n_planes"] == n_ref + 1
    return got, tot


def check_planes(pkg, oracle, contigs, refs, recs, sam, o, kernel, raw=None, want=None, plain=None):
    raw = tl.raw_records(refs, recs) if raw is None else raw
    want = oracle_planes(oracle, contigs, refs, sam, o) if want is None else want
    eng = make_engine(pkg, contigs, refs, o, kernel)
    eng.submit(raw)
    got, tot = check_engine(eng, want, len(refs))
    eng.close()
    if plain is None:
        e2 = make_engine(pkg, contigs, refs, o, kernel, per_contig=False)
        e2.submit(raw)
        plain = e2.finish()
        e2.close()
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev)
    drop = ("slow_path",)
    assert {k: v for k, v in tot.stats.items() if k not in drop} == {k: v for k, v in plain.stats.items() if k not in drop}
    return got, tot


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(7301, 4000, contig_lens=LENS)
    sam = tmp_path_factory.mktemp("percontig") / "all.sam"
    tl.write_sam(sam, refs, recs)
    return contigs, refs, recs, sam, tl.raw_records(refs, recs)


@pytest.fixture(scope="module")
def fuzz_want(oracle, fuzz):
    """the expectation at -r 15 and -r 40, computed once"""
    contigs, refs, recs, sam, _ = fuzz
    return {n: oracle_planes(oracle, contigs, refs, sam, tl.PssOpts(region_len=n)) for n in (15, 40)}


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_planes_match_oracle(pkg, oracle, fuzz, fuzz_want, kernel):
    contigs, refs, recs, sam, raw = fuzz
    got, _ = check_planes(pkg, oracle, contigs, refs, recs, sam, tl.PssOpts(region_len=15), KERNELS[kernel], raw, fuzz_want[15])
    names = [nm for nm, _ in refs]
    assert sorted(got) == list(range(len(LENS)))                    # every contig of the FASTA holds something ...
    assert names.index("chrMissing") not in got and len(refs) not in got   # ... the name it lacks and "*" do not
    rng = np.random.default_rng(310 + KERNELS[kernel])
    for n in (15, 25):
        o = tl.random_pss_opts(rng)
        o.region_len = n
        check_planes(pkg, oracle, contigs, refs, recs, sam, o, KERNELS[kernel], raw)


@pytest.mark.parametrize("n", [15, 40])
@pytest.mark.parametrize("slots", ["1", "2", None])
def test_slot_machinery(pkg, oracle, fuzz, fuzz_want, monkeypatch, slots, n):
    """five contigs mixed in every tile of 64 reads, workgroups that walk several tiles: with one or two slots nearly every
    tile has reads that find none (direct adds, flush and empty); -r 40: a later row pass"""
    contigs, refs, recs, sam, raw = fuzz
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_GRID_WGS", "6")
    if slots:
        monkeypatch.setenv("PSSBAM_CONTIG_SLOTS", slots)
    check_planes(pkg, oracle, contigs, refs, recs, sam, tl.PssOpts(region_len=n), pkg.KERNEL_TILED, raw, fuzz_want[n])


@pytest.mark.parametrize("n", [15, 40])
def test_all_reads_on_one_contig(pkg, oracle, fuzz, tmp_path, monkeypatch, n):
    """no miss: the one slot is flushed once, when the workgroup is done"""
    contigs, refs, recs, _, _ = fuzz
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_GRID_WGS", "4")
    monkeypatch.setenv("PSSBAM_CONTIG_SLOTS", "1")
    one = [r for r in recs if r.rname == "chrA"]
    sam = tmp_path / "one.sam"
    tl.write_sam(sam, refs, one)
    got, _ = check_planes(pkg, oracle, contigs, refs, one, sam, tl.PssOpts(region_len=n), pkg.KERNEL_TILED)
    assert list(got) == [[nm for nm, _ in refs].index("chrA")]


@pytest.mark.parametrize("evict", ["1", "0"])
@pytest.mark.parametrize("n", [15, 40])
def test_sorted_input(pkg, oracle, fuzz, fuzz_want, monkeypatch, evict, n):
    """coordinate-sorted records, two slots: a workgroup meets one contig after the other, and the full table is emptied
    behind a tile that used one slot (PSSBAM_CONTIG_EVICT=0: only when a read found none)"""
    contigs, refs, recs, sam, _ = fuzz
    order = {nm: k for k, (nm, _) in enumerate(refs)}
    by_pos = sorted(recs, key=lambda r: (order.get(r.rname, len(refs)), r.pos))
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_GRID_WGS", "6")
    monkeypatch.setenv("PSSBAM_CONTIG_SLOTS", "2")
    monkeypatch.setenv("PSSBAM_CONTIG_EVICT", evict)
    check_planes(pkg, oracle, contigs, refs, by_pos, sam, tl.PssOpts(region_len=n), pkg.KERNEL_TILED, None, fuzz_want[n])


def test_staged_prefix_overflow(pkg, oracle, fuzz, fuzz_want, monkeypatch):
    """records longer than the staged prefix take the one-lane path straight into their planes"""
    contigs, refs, recs, sam, raw = fuzz
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    for n in (15, 40):
        _, tot = check_planes(pkg, oracle, contigs, refs, recs, sam, tl.PssOpts(region_len=n), pkg.KERNEL_TILED, raw, fuzz_want[n])
        assert tot.stats["slow_path"] > 0


def _many_refs_dataset(seed):
    """210 header names; the six real contigs at refIDs 0, 63, 64, 65, 199, 130 and one FASTA contig named "*" that
    receives the refID -1 records"""
    contigs, _, recs = tl.fuzz_dataset(seed, 4000, contig_lens=(5000, 1200, 300, 900, 700, 2500))
    refs = [(f"unplaced_{i:03d}", 1000 + i) for i in range(210)]
    for (nm, s), k in zip(contigs, [0, 63, 64, 65, 199, 130]):
        refs[k] = (nm, len(s))
    refs[7] = ("chrMissing", 4000)   # every RNAME must be a header name: a BAM writes any other one as refID -1
    rng = np.random.default_rng(seed)
    contigs = contigs + [("*", tl.random_contig(rng, 3000))]
    for r in recs:
        if r.rname == "*" and r.pos > 0:
            r.pos = min(r.pos, 2000)
        elif rng.random() < 0.03:
            r.rname = "unplaced_100"
    return contigs, refs, recs


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_past_64_references(pkg, oracle, tmp_path, kernel):
    """refIDs below and above REF_LDS_ENTRIES, and plane n_ref: the oracle on the contig named "*" """
    contigs, refs, recs = _many_refs_dataset(7302)
    sam = tmp_path / "a.sam"
    tl.write_sam(sam, refs, recs)
    got, _ = check_planes(pkg, oracle, contigs, refs, recs, sam, tl.PssOpts(region_len=20), KERNELS[kernel])
    assert sorted(got) == [0, 63, 64, 65, 130, 199, 210]


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_read_group_filter(pkg, oracle, kernel, tmp_path):
    """-A with -R: the planes of the records -R keeps"""
    contigs, refs, recs = tl.fuzz_dataset(7303, 3000, contig_lens=LENS, with_rg=True)
    keep = [r for r in recs if ("RG", "Z", "grpA") in r.tags]
    sam = tmp_path / "keep.sam"
    tl.write_sam(sam, refs, keep)
    o = tl.PssOpts(region_len=25)
    want = oracle_planes(oracle, contigs, refs, sam, o)
    o_rg = tl.PssOpts(**{**pss_dict(o), "read_group": "grpA"})
    eng = make_engine(pkg, contigs, refs, o_rg, KERNELS[kernel])
    eng.submit(tl.raw_records(refs, recs))
    _, tot = check_engine(eng, want, len(refs))
    assert tot.stats["rg_dropped"] == len(recs) - len(keep)
    eng.close()


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_min_base_quality(pkg, oracle, fuzz, kernel, tmp_path):
    """-A with -Q 20: the planes of the input with the bases below Q20 replaced by N"""
    contigs, refs, recs, _, raw = fuzz
    sam = tmp_path / "masked.sam"
    bq.write_masked_sam(sam, refs, recs, 20)
    o = tl.PssOpts(region_len=15)
    want = oracle_planes(oracle, contigs, refs, sam, o)
    eng = make_engine(pkg, contigs, refs, o, KERNELS[kernel], min_base_qual=20)
    eng.submit(raw)
    check_engine(eng, want, len(refs))
    eng.close()


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_regions(pkg, oracle, fuzz, kernel, tmp_path):
    """-A with -T: the planes of the input reduced to the records that meet an interval"""
    contigs, refs, recs, _, raw = fuzz
    ivs = rl.fuzz_intervals(7304, contigs, recs) + [("tiny.4", 100, 500), ("tiny.5", 0, 350)]
    sam = tmp_path / "reduced.sam"
    kept = rl.write_reduced_sam(sam, refs, recs, ivs)
    assert 0 < len(kept) < len(recs)
    o = tl.PssOpts(region_len=25)
    want = oracle_planes(oracle, contigs, refs, sam, o)
    eng = make_engine(pkg, contigs, refs, o, KERNELS[kernel])
    eng.set_regions(*rl.to_arrays(ivs))
    eng.submit(raw)
    check_engine(eng, want, len(refs))
    eng.close()


def test_equals_contig_sets_of_one_contig_each(pkg, fuzz):
    """the same engine build with -C, one set per header name: every plane equals the set's tables"""
    contigs, refs, recs, _, raw = fuzz
    o = tl.PssOpts(region_len=25, min_mq=5)
    names = [nm for nm, _ in refs]
    eng = make_engine(pkg, contigs, refs, o, pkg.KERNEL_TILED, per_contig=False, contig_sets={nm: [nm] for nm in names})
    eng.submit(raw)
    sets = eng.finish_sets()
    eng.close()
    eng = make_engine(pkg, contigs, refs, o, pkg.KERNEL_TILED)
    eng.submit(raw)
    got = eng.finish_contigs()
    for k, nm in enumerate(names):
        f, r = plane(eng, k)
        assert np.array_equal(f, sets[nm].fwd) and np.array_equal(r, sets[nm].rev), nm
        assert (k in got) == bool(sets[nm].fwd.any() or sets[nm].rev.any())
    eng.close()


def test_same_name_twice_keeps_separate_planes(pkg, oracle, fuzz, fuzz_want):
    """two refIDs that carry the same name: the records of each stay in its own plane"""
    contigs, refs, recs, _, _ = fuzz
    names = [nm for nm, _ in refs]
    twice = refs + [("chrA", dict(refs)["chrA"])]
    idx = {nm: i for i, (nm, _) in enumerate(refs)}
    rng = np.random.default_rng(5)
    second = [r.rname == "chrA" and rng.random() < 0.5 for r in recs]
    raw = np.frombuffer(b"".join(tl.bam_record(r, {**idx, "chrA": len(refs)} if s else idx) for r, s in zip(recs, second)), dtype=np.uint8)
    eng = make_engine(pkg, contigs, twice, tl.PssOpts(region_len=15), pkg.KERNEL_TILED)
    eng.submit(raw)
    got = eng.finish_contigs()
    a, b = names.index("chrA"), len(refs)
    assert got[a].fwd.any() and got[b].fwd.any()
    assert np.array_equal(got[a].fwd + got[b].fwd, fuzz_want[15][a][0]) and np.array_equal(got[a].rev + got[b].rev, fuzz_want[15][a][1])
    eng.close()


def test_compressed_feed(pkg, oracle, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(7305, 4000, contig_lens=LENS)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    sam = tmp_path / "all.sam"
    tl.write_sam(sam, refs, recs)
    o = tl.PssOpts(region_len=15, min_mq=5)
    want = oracle_planes(oracle, contigs, refs, sam, o)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_per_contig(True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    _, tot = check_engine(eng, want, len(refs))
    assert eng.feed_status()["flags"] == 0 and tot.stats["records"] == len(recs)
    eng.close()


def test_rules(pkg, oracle, fuzz, fuzz_want):
    E = pkg.PssbamError
    contigs, refs, recs, sam, raw = fuzz
    names = [nm for nm, _ in refs]
    with pytest.raises(E):                                  # k-mer tables are not split
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), per_contig=True)
    with pytest.raises(E):
        pkg.Engine(kmer=dict(klen=4), per_contig=True)
    others = {"read_groups": ["a"], "length_bins": [30], "contig_sets": {"x": ["chrA"]}, "length_hist": 100, "site_context": "cpg",
              "end_condition": (1, 13, 13), "gapped": True}
    setters = {"read_groups": lambda e: e.set_read_groups(["a"]), "length_bins": lambda e: e.set_length_bins([30]),
               "contig_sets": lambda e: e.set_contig_sets({"x": ["chrA"]}), "length_hist": lambda e: e.set_length_histogram(100),
               "site_context": lambda e: e.set_site_context("cpg"), "end_condition": lambda e: e.set_end_condition(1, 13, 13),
               "gapped": lambda e: e.set_gapped(True)}
    for key, val in others.items():
        eng = pkg.Engine(pss=dict(region_len=5), **{key: val})
        with pytest.raises(E):                              # the other setting is on
            eng.set_per_contig(True)
        assert not eng.per_contig
        eng.close()
        eng = pkg.Engine(pss=dict(region_len=5), per_contig=True)
        with pytest.raises(E):                              # and the other way round
            setters[key](eng)
        eng.close()
    # goes with a read group filter, a minimum base quality and regions; off again: the engine without the setting
    eng = pkg.Engine(pss=dict(region_len=5), read_group="grpA", min_base_qual=20, per_contig=True)
    eng.set_regions(["chrA"], [0], [0], [100])
    eng.set_per_contig(False)
    assert not eng.per_contig and eng.counter_layout()["n_u64"] == eng.counters_device()[1]
    eng.set_length_histogram(50)                            # legal again
    eng.close()
    o = tl.PssOpts(region_len=15)
    want = fuzz_want[15]

    def same(eng):
        got = eng.finish_contigs()
        return sorted(got) == sorted(want) and all(np.array_equal(got[k].fwd, want[k][0]) and np.array_equal(got[k].rev, want[k][1]) for k in want)

    # set after set_references; ESTATE once records have been tallied; survives reset; off after reset
    eng = pkg.Engine(pss=pss_dict(o))
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references(names)
    eng.set_per_contig(True)
    assert eng.counter_layout()["n_u64"] == eng.counters_device()[1]
    eng.submit(raw)
    assert same(eng)
    for on in (True, False):
        with pytest.raises(E):
            eng.set_per_contig(on)
    eng.reset()
    assert eng.per_contig and not eng.finish_contigs()
    eng.submit(raw)
    assert same(eng)
    with pytest.raises(E):                                  # a range outside the planes
        eng.finish_contigs(first=len(refs), n=2)
    eng.reset()
    eng.set_per_contig(False)
    eng.submit(raw)
    plain = eng.finish()
    with pytest.raises(E):
        eng.finish_contigs()
    eng.close()
    # set before the references are known: sized at set_references, and again by one with another count
    eng = pkg.Engine(pss=pss_dict(o), per_contig=True)
    assert eng.counter_layout()["n_u64"] == eng.counters_device()[1]
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references(names[:2])
    assert eng.counter_layout()["n_u64"] == eng.counters_device()[1]
    eng.set_references(names)
    assert eng.counter_layout()["n_u64"] == eng.counters_device()[1]
    eng.submit(raw)
    assert same(eng)
    tot = eng.finish()
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev)
    # the reference list grows after records have been tallied (the SAM-text reader): the planes keep their contents
    eng.set_references(names + ["late_1", "late_2"])
    assert eng.counter_layout()["n_u64"] == eng.counters_device()[1]
    assert same(eng)
    with pytest.raises(E):                                  # ... but it cannot shrink
        eng.set_references(names)
    eng.close()
    # a bound block: the setting is refused, and a bound per-contig block refuses another reference count
    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):
        eng.set_per_contig(True)
    eng.close()
    other.close()
    eng, other = (make_engine(pkg, contigs, refs, tl.PssOpts(region_len=5), pkg.KERNEL_TILED) for _ in range(2))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):
        eng.set_references(names + ["one_more"])
    eng.set_references(names)                               # the same count: fine
    eng.close()
    other.close()


# ---- the command line ----------------------------------------------------------------------------------------------

def test_cli_A_with_R(pkg, tmp_path):
    """-A -R <ID>: the two ordinary files are those of -R alone, every contig's rows those of -C -R with one contig per
    label, and the contigs' tables sum to the totals"""
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    contigs, refs, recs = tl.fuzz_dataset(7307, 3000, contig_lens=LENS, with_rg=True)
    tl.write_fasta(tmp_path / "g.fa", contigs)
    tl.write_bam(tmp_path / "in.bam", refs, recs, rng=np.random.default_rng(4))
    names = [nm for nm, _ in refs]
    (tmp_path / "map.tsv").write_text("".join(f"{nm}\tL{k}\n" for k, nm in enumerate(names)))
    o = tl.PssOpts(region_len=15)

    def pss_bam(prefix, *more):
        pr = subprocess.run([str(exe), "-F", "g.fa", "-B", "in.bam", "-o", prefix, "-R", "grpA", *more] + o.argv(), capture_output=True,
                            text=True, timeout=300, cwd=tmp_path)
        assert pr.returncode == 0, pr.stderr
        return pr

    pr = pss_bam("a", "-A")
    assert " -R grpA " in pr.stderr.splitlines()[0] and pr.stderr.splitlines()[0].endswith(" -A")
    pss_bam("r")
    pss_bam("c", "-C", "map.tsv")
    for kind in ("counts", "rates"):
        assert (tmp_path / f"a.pss.{kind}.txt").read_text() == (tmp_path / f"r.pss.{kind}.txt").read_text().replace("OUT: r.", "OUT: a.")
    _, order, rows = parse_contigs((tmp_path / "a.pss.contigs.txt").read_text())
    assert order == [nm for nm, _ in contigs]
    tf, tr = tl.parse_counts_text((tmp_path / "a.pss.counts.txt").read_text())
    sf, sr = np.zeros_like(tf), np.zeros_like(tr)
    for k, nm in enumerate(names):
        text = (tmp_path / f"c.L{k}.pss.counts.txt").read_text()
        f, r = tl.parse_counts_text(text)
        assert (rows[nm] == body(text)) if nm in rows else not (f.any() or r.any()), nm
        sf, sr = sf + f, sr + r
    assert np.array_equal(sf, tf) and np.array_equal(sr, tr) and tf.any()
    # -R took records away: the tables of all reads hold more
    pr = subprocess.run([str(exe), "-F", "g.fa", "-B", "in.bam", "-o", "all"] + o.argv(), capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert pr.returncode == 0, pr.stderr
    assert tl.parse_counts_text((tmp_path / "all.pss.counts.txt").read_text())[0].sum() > tf.sum()


CLI_MODES = {
    "bam_device_feed": ("bam", {}),
    "bam_host_reader": ("bam", {"PSSBAM_DEVICE_INFLATE": "0"}),
    "sam": ("sam", {}),
    "bam_two_gpus": ("bam", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}),
}


def body(counts_text: str) -> list:
    """the rows of a counts file: forward -2 .. N-1, reverse N-1 .. 0, 1, 2"""
    return [ln for ln in counts_text.splitlines() if ln and not ln.startswith("#")]


def parse_contigs(text: str):
    """the contigs file -> (header lines, [names in order of appearance], {name: rows without the two leading fields})"""
    lines = text.splitlines()
    head, rows, order = lines[:5], {}, []
    for ln in lines[5:]:
        nm, table, rest = ln.split("\t", 2)
        assert table in ("fwd", "rev")
        if nm not in rows:
            order.append(nm)
            rows[nm] = {"fwd": [], "rev": []}
        assert table == "fwd" or rows[nm]["fwd"]       # a contig's forward rows come first ...
        assert table == "rev" or not rows[nm]["rev"]
        assert order[-1] == nm                         # ... and its lines are together
        rows[nm][table].append(rest)
    return head, order, {nm: r["fwd"] + r["rev"] for nm, r in rows.items()}


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_A(pkg, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    contigs, refs, recs = tl.fuzz_dataset(7306, 6000, contig_lens=LENS)
    recs = tl.ref_safe(recs)
    run = tmp_path / "run"
    run.mkdir()
    tl.write_fasta(run / "g.fa", contigs)
    aln = tmp_path / f"in.{fmt}"
    if fmt == "bam":
        tl.write_bam(aln, refs, recs, rng=np.random.default_rng(2))
    else:
        tl.write_sam(aln, refs, recs)
    names = [nm for nm, _ in refs]
    (tmp_path / "map.tsv").write_text("".join(f"{nm}\tL{k}\n" for k, nm in enumerate(names)))
    o = tl.PssOpts(region_len=25, min_mq=10, min_read_len=10)
    env = {**os.environ, **extra}

    def pss_bam(cwd: Path, prefix: str, *more, ok=True):
        pr = subprocess.run([str(exe), "-F", "g.fa", "-B", str(aln), "-o", prefix, *more] + o.argv(), capture_output=True,
                            text=True, env=env, timeout=300, cwd=cwd)
        assert (pr.returncode == 0) == ok, pr.stderr
        return pr

    pr = pss_bam(run, "out", "-A")
    assert pr.stderr.splitlines()[0].endswith(" -A")
    assert sorted(p.name for p in run.glob("out.*")) == ["out.pss.contigs.txt", "out.pss.counts.txt", "out.pss.rates.txt"]
    # the two ordinary files: byte-identical to the same command without -A
    plain = tmp_path / "plain"
    plain.mkdir()
    (plain / "g.fa").write_bytes((run / "g.fa").read_bytes())
    pss_bam(plain, "out")
    for kind in ("counts", "rates"):
        assert (plain / f"out.pss.{kind}.txt").read_text() == (run / f"out.pss.{kind}.txt").read_text()
    head, order, rows = parse_contigs((run / "out.pss.contigs.txt").read_text())
    assert head == ["### pss-bam.c v1.2.1:", "### FASTA: g.fa", f"### BAM: {aln}", "### OUT: out.pss.contigs.txt",
                    "### CONTIG TABLE POS AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT"]
    # every contig of the FASTA, in header order; the header name the FASTA lacks and "*" are absent
    assert order == [nm for nm, _ in contigs] == names[:len(contigs)]
    # -C of the same binary with one contig per label
    sets = tmp_path / "sets"
    sets.mkdir()
    (sets / "g.fa").write_bytes((run / "g.fa").read_bytes())
    pss_bam(sets, "out", "-C", str(tmp_path / "map.tsv"))
    for k, nm in enumerate(names):
        ct = body((sets / f"out.L{k}.pss.counts.txt").read_text())
        if nm in rows:
            assert rows[nm] == ct, nm
        else:
            f, r = tl.parse_counts_text((sets / f"out.L{k}.pss.counts.txt").read_text())
            assert not f.any() and not r.any(), nm
    # the reference itself on the FASTA reduced to the contig
    if tl.have_ref() and mode in ("bam_device_feed", "sam"):
        for nm, seq in contigs:
            d = tmp_path / f"ref_{nm}"
            d.mkdir()
            tl.write_fasta(d / "g.fa", [(nm, seq)])
            cwd = os.getcwd()
            os.chdir(d)
            try:
                _, _, wc, _, _ = tl.run_ref_pss(Path("g.fa"), aln, Path("out"), o, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
            finally:
                os.chdir(cwd)
            assert body(wc) == rows[nm], nm
    if mode == "bam_device_feed":   # the exclusive options, and the ones it goes with
        for more in (["-G"], ["-S", "40"], ["-C", str(tmp_path / "map.tsv")], ["-H", "100"], ["-X", "cpg"], ["-E", "ss"], ["-I"]):
            bad = pss_bam(run, "bad", "-A", *more, ok=False)
            assert bad.stderr.startswith("-A (tables per contig) and ") and not list(run.glob("bad.*"))
        (tmp_path / "t.bed").write_text("chrB\t1000\t3000\ntiny.4\t0\t400\n")
        pss_bam(run, "rqt", "-A", "-Q", "20", "-T", str(tmp_path / "t.bed"))
        pss_bam(plain, "rqt", "-Q", "20", "-T", str(tmp_path / "t.bed"))
        assert (plain / "rqt.pss.counts.txt").read_text() == (run / "rqt.pss.counts.txt").read_text()
        _, order, rows = parse_contigs((run / "rqt.pss.contigs.txt").read_text())
        assert order == ["chrB", "tiny.4"]
        tf, tr = tl.parse_counts_text((run / "rqt.pss.counts.txt").read_text())
        parts = [tl.parse_counts_text("\n".join(rows[nm][:27]) + "\n\n\n### Reverse read substitution counts and base context\n" +
                                       "\n".join(rows[nm][27:]) + "\n")
                 for nm in order]
        assert np.array_equal(sum(p[0] for p in parts), tf) and np.array_equal(sum(p[1] for p in parts), tr)

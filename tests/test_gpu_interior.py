"""pss-bam -W on the GPU: the 4 x 4 substitution table of the read interior, counted in the tally kernels (tally_tiled's
INTERIOR arm; tally_simple and the tiled kernel's one-lane path through count_interior).  The yardstick is interior_lib's
restatement of the definition, which test_interior_host.py holds against the CPU oracle and against the unmodified
reference's golden.  Bit-exact (integer work).

One case of the issue's list is written the way the engine decides today, as the issue's own definition demands ("a record
that enters neither table does not count"): an unpaired record that fails -U is added to NO table, whatever -D says (both
tests are needed for either table), so it does not count.  The record that fails -U, passes -D and counts once is the
paired one that carries both mate flags: it misses the forward table as read 1 and enters the reverse table as read 2."""
import ctypes as C
import os
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import interior_lib as il
import mismatch_lib as ml
import pssbam_testlib as tl
import regions_lib as rl
import site_context_lib as sc
from test_gpu_length_hist import pss_dict, same_but_slow_path
from test_gpu_tile_loop import assert_every_tile_overflows

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
KERNELS = ["SIMPLE", "TILED"]
LENGTHS = (1, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 150)
MARGINS = (0, 1, 7, 8, 9, 15, 16, 31, 32, 33)
OFF_DIAGONAL = [c for c in range(16) if c // 4 != c % 4]


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def kern(pkg, name):
    return {"SIMPLE": pkg.KERNEL_SIMPLE, "TILED": pkg.KERNEL_TILED, "AUTO": pkg.KERNEL_AUTO}[name]


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, d, q: int = 0, regions=None, **kw):
    """-> (totals, (table, reads) or None, n_u64)"""
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, interior=d, min_base_qual=q, **kw)
    assert eng.interior == d
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if regions is not None:
        eng.set_regions(*rl.to_arrays(regions))
    if recs:
        eng.submit(tl.raw_records(refs, recs))
    got = eng.finish_interior() if d is not None else None
    tot = eng.finish()
    n_u64 = eng.counters_device()[1]
    eng.close()
    if got is not None:
        assert got[0].shape == (16,) and got[0].dtype == np.uint64
    return tot, got, n_u64


def check(pkg, contigs, refs, recs, o, kernel: str, d: int, q: int = 0, ivs=None, **kw):
    """one engine run against the restatement (on the records that meet a region, where regions are given)"""
    want = il.interior(recs if ivs is None else rl.reduce_recs(recs, ivs), contigs, d, o, q)
    tot, (table, reads), _ = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), d, q, ivs, **kw)
    assert np.array_equal(table, want[0]), (d, kernel, table.astype(np.int64) - want[0].astype(np.int64))
    assert reads == want[1] and tot.stats["pss_ok"] == want[2], (reads, want[1:], tot.stats)
    return tot, table, reads, want


# ---- 1. lengths, margins, alignment, the edges of I ---------------------------------------------------------------------

def clean():
    text = il.clean_contig(9000, seed=31)
    return [("c", text)], [("c", len(text))], text


def edge_records(text: str, L: int, d: int):
    """<L>M records at every start mod 8, with names of every length mod 4 (the record's offset in the block): untouched, one
    transversion at each edge of I (d - 1 and L - d outside, d and L - d - 1 inside), either side of the lanes' cut, at the
    read's two ends, and one every third base"""
    cut = il.lane_cut(d, L)
    spots = sorted({p for p in (0, L - 1, d - 1, d, L - d - 1, L - d, cut - 1, cut, cut - 8, cut + 7, (d & ~7) + 8) if 0 <= p < L})
    recs, n = [], 0
    for a in range(8):
        s = 40 + 21 * L + a
        for subs in [[]] + [[p] for p in spots] + [list(range(0, L, 3))]:
            n += 1
            recs.append(il.with_mismatches(text, s, L, subs, name=f"e{n:03d}" + "x" * (n % 4), flag=16 if n % 3 == 0 else 0))
    return recs


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d", MARGINS)
def test_lengths_and_margins(pkg, d, kernel):
    """every length on its own run: L = 2d - 1 and 2d give an empty interior, 2d + 1 and 2d + 2 one and two positions"""
    contigs, refs, text = clean()
    o = tl.PssOpts(region_len=0)
    for L in sorted({*LENGTHS, *(x for x in (2 * d - 1, 2 * d, 2 * d + 1, 2 * d + 2) if x >= 1)}):
        recs = edge_records(text, L, d)
        _, table, reads, want = check(pkg, contigs, refs, recs, o, kernel, d)
        assert want[2] == len(recs) and reads == (len(recs) if L > 2 * d else 0) and int(table.sum()) == len(recs) * max(L - 2 * d, 0)
        if L > 2 * d + 2:
            assert sum(int(table[c]) for c in OFF_DIAGONAL) >= 16       # the in-positions were seen


def test_edge_records_hold_what_they_claim():
    """(no GPU work) the hand-built records against the definition"""
    _, _, text = clean()
    ctg = {"c": text}
    for d, L in ((8, 33), (15, 64), (0, 9), (33, 150)):
        recs = edge_records(text, L, d)
        assert {(r.pos - 1) % 8 for r in recs} == set(range(8)) and {len(r.qname) % 4 for r in recs} == {0, 1, 2, 3}
        assert {r.flag for r in recs} == {0, 16}
        per = [int(sum(il.record_interior(r, ctg, d)[0][c] for c in OFF_DIAGONAL)) for r in recs[:8]]
        assert per[0] == 0 and 1 in per[1:] and (d == 0 or 0 in per[1:])   # a transversion inside I is seen, one outside is not
        one = il.with_mismatches(text, 100, L, [d]) if L > 2 * d else None
        if one is not None:
            assert il.record_interior(one, ctg, d)[0][OFF_DIAGONAL].sum() == 1
            if d:
                assert il.record_interior(il.with_mismatches(text, 100, L, [d - 1, L - d]), ctg, d)[0][OFF_DIAGONAL].sum() == 0


# ---- 2. pairs, strands, letters, short SEQ, mates, -Q, -T --------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_all_pairs_on_both_strands(pkg, kernel):
    """one record per (read base, reference base, strand): the record's own bin holds it, a reverse read in 15 - bin"""
    contigs, refs, text = clean()
    d, L = 8, 40
    for flag in (0, 16):
        for rd in range(4):
            for rf in range(4):
                s = next(p for p in range(200 + 50 * (4 * rd + rf), 8000) if text[p + 20] == "ACGT"[rf])
                rec = il.read_on(text, s, L, {20: "ACGT"[rd]}, flag=flag)
                _, table, reads, _ = check(pkg, contigs, refs, [rec], tl.PssOpts(region_len=5), kernel, d)
                cell = 4 * rd + rf
                rest = il.record_interior(il.read_on(text, s, L, flag=flag), {"c": text}, d)[0]
                base = 5 * rf
                rest[15 - base if flag else base] -= 1                  # position 20 without the substitution
                want = rest.copy()
                want[15 - cell if flag else cell] += 1
                assert reads == 1 and np.array_equal(table, want)


@pytest.mark.parametrize("kernel", KERNELS)
def test_letters_that_never_count_and_short_seq(pkg, kernel):
    clean_text = il.clean_contig(3000, seed=41)
    odd = list(il.clean_contig(3000, seed=42))
    odd[1000:1100] = "".join(odd[1000:1100]).lower()                     # lower case: folded, counts like upper case
    for p in range(1200, 1245, 7):
        odd[p] = "N"
    for p in range(1203, 1245, 7):
        odd[p] = "Y"
    odd = "".join(odd)
    contigs = [("c", clean_text), ("odd", odd)]
    refs = [(nm, len(t)) for nm, t in contigs]
    recs = []
    for a in range(8):
        s = 100 + 50 * a + a
        recs.append(il.read_on(clean_text, s, 40, {3: "N", 11: "R", 20: "=", 39: "N"}, name=f"a{a}"))
        recs.append(il.read_on(odd, 1190 + a, 60, name=f"b{a}", rname="odd", flag=16 * (a & 1)))
        recs.append(il.read_on(odd, 1190 + a, 60, {i: "A" for i in range(60)}, name=f"c{a}", rname="odd"))
        recs.append(il.with_mismatches(odd, 1010 + a, 50, [0, 17, 49], name=f"d{a}", rname="odd"))
        for n_seq in (33, 40, 41):                                       # l_seq < L: a first mate whose |TLEN| and CIGAR say 50
            recs.append(il.with_mismatches(clean_text, 2000 + 11 * a, 50, [5, n_seq - 1], name=f"s{a}", flag=0x1 | 0x2 | 0x40, tlen=50, seq_len=n_seq))
    for d in (0, 5, 9):
        _, table, reads, want = check(pkg, contigs, refs, recs, tl.PssOpts(region_len=5), kernel, d)
        assert want[2] == len(recs) == reads
    per = il.record_interior(recs[0], dict(contigs), 0)[0]
    assert per.sum() == 40 - 4 and il.record_interior(recs[1], dict(contigs), 0)[0].sum() < 60 - 10


@pytest.mark.parametrize("kernel", KERNELS)
def test_mates_and_flags(pkg, kernel):
    """a read 1 and a read 2 count once each; an unpaired read that fails -U enters no table and does not count, the paired
    record with both mate flags that fails -U and passes -D counts once (reverse table); failing both does not; every reject
    flag does not"""
    contigs, refs, text = clean()
    L, d = 44, 6
    o = tl.PssOpts(region_len=5, up_ctx="A", down_ctx="C")
    s_ok = next(p for p in range(100, 8000) if text[p - 1] == "A" and text[p + L] == "C")
    s_noU = next(p for p in range(100, 8000) if text[p - 1] != "A" and text[p + L] == "C")
    s_none = next(p for p in range(100, 8000) if text[p - 1] != "A" and text[p + L] != "C")
    P = 0x1 | 0x2
    groups = {
        "read1": ([il.with_mismatches(text, s_ok, L, [10], flag=P | 0x40, tlen=L)], 1),
        "read2": ([il.with_mismatches(text, s_ok, L, [10], flag=P | 0x80, tlen=-L)], 1),
        "unpaired": ([il.with_mismatches(text, s_ok, L, [10])], 1),
        "unpaired_fails_U": ([il.with_mismatches(text, s_noU, L, [10])], 0),
        "both_mate_flags_fails_U_passes_D": ([il.with_mismatches(text, s_noU, L, [10], flag=P | 0xC0, tlen=L)], 1),
        "read1_fails_U": ([il.with_mismatches(text, s_noU, L, [10], flag=P | 0x40, tlen=L)], 0),
        "fails_both": ([il.with_mismatches(text, s_none, L, [10]), il.with_mismatches(text, s_none, L, [10], flag=P | 0xC0, tlen=L)], 0),
        "reject_flags": ([il.with_mismatches(text, s_ok, L, [10], flag=f, name=f"f{f}") for f in (0x4, 0x100, 0x200, 0x400, 0x800)], 0),
        "low_mapq": ([il.with_mismatches(text, s_ok, L, [10], mapq=3)], 0),
    }
    o = replace(o, min_mq=10)
    for name, (recs, n) in groups.items():
        tot, table, reads, want = check(pkg, contigs, refs, recs, o, kernel, d)
        assert reads == n and int(table.sum()) == n * (L - 2 * d) and int(table[OFF_DIAGONAL].sum()) == n, name
        assert tot.stats["pss_ok"] == n, name
    every = [r for recs, _ in groups.values() for r in recs]
    _, table, reads, _ = check(pkg, contigs, refs, every, o, kernel, d)
    assert reads == 4


@pytest.mark.parametrize("kernel", KERNELS)
def test_min_base_quality(pkg, kernel):
    """-Q 20: a low quality at a position of I takes that position out, one outside I changes nothing; 0xFF quality bytes
    mask nothing (behind a first byte that is present: a record whose whole QUAL is absent is dropped by the parser)"""
    contigs, refs, text = clean()
    L, d = 50, 7
    recs = []
    for a in range(8):
        s = 300 + 60 * a + a
        for j, low in enumerate(([], [d], [d - 1], [L - d - 1], [L - d], [20, 21, 30], list(range(L)))):
            qual = "".join("#" if i in low else "5" for i in range(L))
            recs.append(replace(il.with_mismatches(text, s, L, [d, 20, L - d - 1], name=f"q{a}{j}" + "x" * (j % 4), flag=16 * (j & 1)), qual=qual))
        recs.append(replace(il.with_mismatches(text, s, L, [d, 20], name=f"n{a}"), qual="5" + chr(0xFF + 33) * (L - 1)))
    tot, table, reads, want = check(pkg, contigs, refs, recs, tl.PssOpts(region_len=5), kernel, d, q=20)
    plain = il.interior(recs, contigs, d)
    assert reads == len(recs) and int(plain[0].sum()) - int(table.sum()) == 8 * (1 + 1 + 3 + (L - 2 * d))
    assert np.array_equal(check(pkg, contigs, refs, recs, tl.PssOpts(region_len=5), kernel, d, q=3)[1], table)      # Phred 2 is below 3 as well
    assert np.array_equal(check(pkg, contigs, refs, recs, tl.PssOpts(region_len=5), kernel, d, q=2)[1], plain[0])


# ---- 3. random records ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fuzz():
    return tl.fuzz_dataset(7411, 2000)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d", [0, 15])
@pytest.mark.parametrize("n", [0, 15, 30])
def test_random_records(pkg, fuzz, n, d, kernel):
    contigs, refs, recs = fuzz
    tot, table, reads, want = check(pkg, contigs, refs, recs, tl.PssOpts(region_len=n), kernel, d)
    assert 200 < reads <= want[2] and table[OFF_DIAGONAL].all() and int(table.sum()) > 5000
    plain, _, _ = run_engine(pkg, contigs, refs, recs, tl.PssOpts(region_len=n), kern(pkg, kernel), None)
    same_but_slow_path(tot, plain)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("base", ["setA", "setD"])
def test_golden_sets(pkg, base, kernel):
    contigs = sc.read_fasta(GOLD / f"{base}.fa")
    refs, recs = ml.read_sam(GOLD / f"{base}.sam")
    for d in (0, 15):
        _, table, reads, _ = check(pkg, contigs, refs, recs, tl.PssOpts(), kernel, d)
        if (base, d) == ("setD", 15):
            gold = il.parse_golden((GOLD / "interior15_setD.txt").read_text())
            assert np.array_equal(table, gold["table"]) and reads == gold["reads"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_regions_and_base_quality_on_random_records(pkg, fuzz, kernel):
    """-T: a record that meets no region does not count; with -Q 20 on top"""
    contigs, refs, recs = fuzz
    ivs = rl.fuzz_intervals(7411, contigs, recs)
    o = tl.PssOpts(region_len=15)
    tot, table, reads, want = check(pkg, contigs, refs, recs, o, kernel, 5, ivs=ivs)
    whole = il.interior(recs, contigs, 5, o)
    assert 0 < reads < whole[1] and tot.stats["pss_filtered"] > 0
    _, tq, rq, _ = check(pkg, contigs, refs, recs, o, kernel, 5, q=20, ivs=ivs)
    assert rq == reads and 0 < int(tq.sum()) < int(table.sum())


@pytest.mark.parametrize("kernel", KERNELS)
def test_identity_with_the_mismatch_histogram(pkg, kernel):
    """two engines on the same records: with d = 0 the off-diagonal bins sum to the mismatches of the reads that were tallied,
    each read once -- first mates from mf, second mates from mr, unpaired reads from either (every read here stays inside the
    histogram's limit)"""
    contigs, refs, recs = tl.fuzz_dataset(7412, 1500)
    ctg = dict(contigs)
    assert max(m for m in (ml.mismatches(r, ctg) for r in recs) if m is not None) <= 254
    o = tl.PssOpts(region_len=15)
    _, (table, reads), _ = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), 0)
    total = 0
    for part, pick in (([r for r in recs if not r.flag & 1], 0), ([r for r in recs if r.flag & 1], None)):
        eng = pkg.Engine(pss=pss_dict(o), kernel=kern(pkg, kernel), mismatches=(255, -1, 0))
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        eng.submit(tl.raw_records(refs, part))
        mf, mr = eng.finish_mismatches()
        eng.close()
        hist = mf if pick == 0 else mf + mr                              # a paired record is in exactly one of the two
        total += int((np.arange(257, dtype=np.uint64) * hist).sum())
    assert int(table[OFF_DIAGONAL].sum()) == total > 100


# ---- 4. several tiles per workgroup, the one-lane path, the compressed feed ----------------------------------------------

SHAPES = {
    "one_wg": {"PSSBAM_GRID_WGS": "1", "PSSBAM_TILE_READS": "48"},
    "three_wg": {"PSSBAM_GRID_WGS": "3", "PSSBAM_TILE_READS": "48"},
    "xcd8": {"PSSBAM_XCD_MAP": "1", "PSSBAM_GRID_WGS": "8", "PSSBAM_TILE_READS": "48"},
    "two_wg_overflow": {"PSSBAM_GRID_WGS": "2", "PSSBAM_TILE_READS": "64", "PSSBAM_PIECES": "5"},
    "simple_one_block": {"PSSBAM_SIMPLE_BLOCKS": "1"},
}


@pytest.fixture(scope="module")
def tiles():
    contigs, refs, recs = tl.fuzz_dataset(9601, 3200)
    assert_every_tile_overflows(tl.raw_records(refs, recs))      # with 5 pieces every tile of 64 holds an overflow record
    return contigs, refs, recs


@pytest.mark.parametrize("q", [0, 20])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_several_tiles_per_workgroup(pkg, tiles, monkeypatch, shape, q):
    """the LDS words must survive the tile loop, and the one-lane path adds the same counts"""
    for key, v in SHAPES[shape].items():
        monkeypatch.setenv(key, v)
    kernel = "SIMPLE" if shape == "simple_one_block" else "TILED"
    tot, table, reads, _ = check(pkg, *tiles, tl.PssOpts(region_len=15), kernel, 5, q=q)
    assert reads > 500
    if shape == "two_wg_overflow":
        assert tot.stats["slow_path"] >= 50


def test_one_workgroup_walks_more_than_8192_tiles(pkg, monkeypatch):
    """the LDS words are handed to the counter block every 8192 tiles of a workgroup (so that a u32 word cannot wrap): one
    workgroup, tiles of 16 reads, 8 200 tiles -- the counts on both sides of the hand-over add up"""
    monkeypatch.setenv("PSSBAM_GRID_WGS", "1")
    monkeypatch.setenv("PSSBAM_TILE_READS", "16")
    contigs, refs, text = clean()
    recs = [il.with_mismatches(text, 100 + 13 * j, 24, [j % 24], name=f"t{j:03d}", flag=16 * (j & 1)) for j in range(160)]
    o, d, times = tl.PssOpts(region_len=5), 3, 820
    want = il.interior(recs, contigs, d, o)
    block = np.tile(tl.raw_records(refs, recs), times)
    eng = pkg.Engine(pss=pss_dict(o), kernel=pkg.KERNEL_TILED, interior=d)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(block)
    table, reads = eng.finish_interior()
    tot = eng.finish()
    eng.close()
    assert tot.stats["records"] == 160 * times > 8192 * 16 and tot.stats["pss_ok"] == want[2] * times
    assert np.array_equal(table, want[0] * np.uint64(times)) and reads == want[1] * times == 160 * times


def test_submit_bgzf(pkg, fuzz, tmp_path):
    """the compressed feed (device-indexed blocks) goes through the same launches; the setting follows feed_open"""
    contigs, refs, recs = fuzz
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    o = tl.PssOpts(region_len=15)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_interior(15)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    table, reads = eng.finish_interior()
    tot = eng.finish()
    assert eng.feed_status()["flags"] == 0
    eng.close()
    want = il.interior(recs, contigs, 15, o)
    assert np.array_equal(table, want[0]) and reads == want[1] and tot.stats["pss_ok"] == want[2] and tot.stats["records"] == len(recs)


# ---- 5. off is off, reset, reduce, rules ---------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["AUTO", "SIMPLE", "TILED"])
def test_off_is_off(pkg, fuzz, kernel):
    contigs, refs, recs = fuzz
    o = tl.PssOpts(region_len=15)
    plain, _, n_plain = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), None)
    eng = pkg.Engine(pss=pss_dict(o), kernel=kern(pkg, kernel), interior=4)
    lay = eng.counter_layout()
    assert eng.counters_device()[1] == n_plain + 17 == lay["n_u64"] and lay["interior"] == n_plain and lay["interior_reads"] == n_plain + 16
    eng.set_interior(-1)
    assert eng.interior is None and eng.counters_device()[1] == n_plain == eng.counter_layout()["n_u64"]
    assert "interior" not in eng.counter_layout()
    with pytest.raises(pkg.PssbamError):
        eng.finish_interior()
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    tot = eng.finish()
    eng.close()
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev) and tot.stats == plain.stats
    on, _, n_on = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), 4)      # on: tables and stats are untouched as well
    assert n_on == n_plain + 17
    same_but_slow_path(on, plain)


def test_reset_keeps_the_setting_and_reduce_sums_the_words(pkg, fuzz):
    contigs, refs, recs = fuzz
    o = tl.PssOpts(region_len=15)
    want = il.interior(recs, contigs, 9, o)

    def make():
        eng = pkg.Engine(pss=pss_dict(o), interior=9)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        return eng

    eng = make()
    n = eng.counters_device()[1]
    eng.submit(tl.raw_records(refs, recs))
    with pytest.raises(pkg.PssbamError):                   # records have been tallied
        eng.set_interior(3)
    first = eng.finish_interior()
    eng.reset()
    assert eng.interior == 9 and eng.counters_device()[1] == n
    zt, zr = eng.finish_interior()
    assert not zt.any() and zr == 0
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_interior()
    assert np.array_equal(first[0], want[0]) and np.array_equal(again[0], want[0]) and first[1] == again[1] == want[1]
    eng.reset()
    eng.set_interior(2)                                    # legal again after reset; the block keeps its size
    assert eng.counters_device()[1] == n
    eng.close()

    half = len(recs) // 2
    engs = [make(), make()]
    engs[0].submit(tl.raw_records(refs, recs[:half]))
    engs[1].submit(tl.raw_records(refs, recs[half:]))
    arr = (C.c_void_p * 2)(engs[0]._h, engs[1]._h)
    assert pkg.hip_lib().pssbam_reduce_counters(arr, 2, 0) == 0
    table, reads = engs[0].finish_interior()
    for e in engs:
        e.close()
    assert np.array_equal(table, want[0]) and reads == want[1]


def test_rules(pkg):
    E = pkg.PssbamError
    for bad in (65536, -2, 1 << 20):
        with pytest.raises(E):
            pkg.Engine(pss=dict(region_len=5), interior=bad)
    with pytest.raises(E):                                  # nothing is added to a table on a k-mer engine
        pkg.Engine(kmer=dict(klen=4), interior=4)
    with pytest.raises(E):
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), interior=4)
    with pytest.raises(E):                                  # a read's fate is decided in the one pass that holds all rows
        pkg.Engine(pss=dict(region_len=31), interior=4)
    others = (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]}), dict(per_contig=True), dict(replicates=4),
              dict(length_hist=100), dict(site_context="cpg"), dict(end_condition=(1, 13, 13)), dict(gapped=True),
              dict(mismatches=(4, -1, 0)), dict(mismatches=(0, 2, 0)))
    for kw in others:
        eng = pkg.Engine(pss=dict(region_len=5), **kw)
        with pytest.raises(E):
            eng.set_interior(4)
        assert eng.interior is None
        eng.set_interior(-1)                                # switching off what is off is always legal
        eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), interior=0)
    for setter, args in ((eng.set_read_groups, (["a"],)), (eng.set_length_bins, ([30],)), (eng.set_contig_sets, ({"x": ["chrA"]},)),
                         (eng.set_per_contig, (True,)), (eng.set_replicates, (4,)), (eng.set_length_histogram, (100,)),
                         (eng.set_site_context, ("cpg",)), (eng.set_end_condition, (1, 13, 13)), (eng.set_gapped, (True,)),
                         (eng.set_mismatches, (4, -1, 0)), (eng.set_mismatches, (0, 2, 0))):
        with pytest.raises(E):
            setter(*args)
    assert eng.interior == 0
    eng.set_interior(-1)
    eng.set_length_histogram(100)                           # off again: the others are legal
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=30), read_group="grpA", min_base_qual=10, interior=65535)   # goes with -R, -Q and -r 30
    assert eng.interior == 65535
    eng.close()
    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    dptr, n = other.counters_device()
    eng.bind_counters(dptr, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_interior(4)
    eng.close()
    other.close()


# ---- 6. the command line ---------------------------------------------------------------------------------------------------

def run_cli(pkg, fa, aln, prefix, *more, env=None):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), *more], capture_output=True, text=True,
                          env={**os.environ, **(env or {})}, timeout=300)


@pytest.mark.parametrize("aln", ["setD.bam", "setD.sam"])
def test_cli_against_the_golden(pkg, tmp_path, aln):
    """-W 15 on setD (BAM, and the SAM-text reader): the interior file against the reference's golden, counts and rates files
    byte-equal to the run without -W"""
    fa = GOLD / "setD.fa"
    gold = il.parse_golden((GOLD / "interior15_setD.txt").read_text())
    for tag, args in (("with", ["-W", "15"]), ("without", [])):
        (tmp_path / tag).mkdir()
        pr = run_cli(pkg, fa, GOLD / aln, tmp_path / tag / "out", *args)
        assert pr.returncode == 0, pr.stderr
        assert pr.stderr.splitlines()[0].endswith(" -W 15") == bool(args)
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == ["out.pss.counts.txt", "out.pss.interior.txt", "out.pss.rates.txt"]
    assert sorted(p.name for p in (tmp_path / "without").iterdir()) == ["out.pss.counts.txt", "out.pss.rates.txt"]
    for kind in ("counts", "rates"):
        a, b = ((tmp_path / tag / f"out.pss.{kind}.txt").read_text().replace(f"{tag}/out", "X/out") for tag in ("with", "without"))
        assert a == b, kind
    got = il.parse_interior_file((tmp_path / "with" / "out.pss.interior.txt").read_text())
    assert got["label"] == 15 and np.array_equal(got["table"], gold["table"]) and got["reads"] == gold["reads"] and got["bases"] == gold["bases"]
    assert got["rates"] == il.expected_rates(gold["table"]) and "-Q" not in got["comment"] and " 15 bases" in got["comment"]


def test_cli_with_base_quality_and_two_engines(pkg, fuzz, tmp_path):
    """-W 5 -Q 20, one engine and two engines whose counter blocks are summed: the same three files"""
    contigs, refs, recs = fuzz
    recs = [replace(r, qname=f"{r.qname}.{j}") for j in range(4) for r in tl.ref_safe(recs)]     # a few batches of 1 MiB
    fa, aln = tmp_path / "g.fa", tmp_path / "in.bam"
    tl.write_fasta(fa, contigs)
    tl.write_bam(aln, refs, recs, rng=np.random.default_rng(2))
    outs = {}
    for tag, e in (("one", {}), ("two", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"})):
        pr = run_cli(pkg, fa, aln, tmp_path / "out", "-W", "5", "-Q", "20", env=e)
        assert pr.returncode == 0, pr.stderr
        outs[tag] = {kind: (tmp_path / f"out.pss.{kind}.txt").read_bytes() for kind in ("counts", "rates", "interior")}
    assert outs["one"] == outs["two"]
    got = il.parse_interior_file(outs["one"]["interior"].decode())
    want = il.interior(recs, contigs, 5, tl.PssOpts(), 20)
    assert np.array_equal(got["table"], want[0]) and got["reads"] == want[1] and got["comment"].endswith("(-Q 20)")

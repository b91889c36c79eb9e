"""pss-bam -P on the GPU: the reference base composition around the read ends, counted in the tally kernels (tally_tiled's
COMP arm; tally_simple and the tiled kernel's one-lane path through count_composition).  The yardstick is composition_lib's
restatement of the definition, which test_composition_host.py holds against the rows of the unmodified reference.  Bit-exact
(integer work)."""
import ctypes as C
import os
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import composition_lib as cl
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
WIDTHS = (1, 2, 3, 8, 29, 30)
LENGTHS = (1, 5, 7, 8, 9, 29, 30, 31, 150)
REGION_LENS = (0, 3, 30)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def kern(pkg, name):
    return {"SIMPLE": pkg.KERNEL_SIMPLE, "TILED": pkg.KERNEL_TILED, "AUTO": pkg.KERNEL_AUTO}[name]


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, w, q: int = 0, regions=None, **kw):
    """-> (totals, (c5, c3) or None, n_u64)"""
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, composition=w, min_base_qual=q, **kw)
    assert eng.composition == w
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if regions is not None:
        eng.set_regions(*rl.to_arrays(regions))
    if recs:
        eng.submit(tl.raw_records(refs, recs))
    got = eng.finish_composition() if w is not None else None
    tot = eng.finish()
    n_u64 = eng.counters_device()[1]
    eng.close()
    if got is not None:
        assert all(a.shape == (2 * w, 5) and a.dtype == np.uint64 for a in got)
    return tot, got, n_u64


def rows_exist(recs, contigs, w: int, o: tl.PssOpts):
    """(n5, n3): per row, the records added to the forward / reverse table whose position at that offset exists -- counted
    from coordinates alone, without looking at a letter"""
    ctg = dict(contigs)
    n5, n3 = np.zeros(2 * w, dtype=np.uint64), np.zeros(2 * w, dtype=np.uint64)
    for r in recs:
        f, v = il.tables_entered(r, ctg, o)
        L, s, rev, glen = il.pss_length(r), r.pos - 1, bool(r.flag & 0x10), len(ctg.get(r.rname, ""))
        for n, on, left in ((n5, f, not rev), (n3, v, rev)):
            if on:
                for j in range(-w, min(w, L)):
                    n[j + w] += 0 <= (s + j if left else s + L - 1 - j) < glen
    return n5, n3


def check(pkg, contigs, refs, recs, o, kernel: str, w: int, q: int = 0, ivs=None, expect=None, **kw):
    """one engine run against the restatement (on the records that meet a region, where regions are given; `expect`: the
    records the restatement is taken over, where a filter it does not know is in force)"""
    kept = expect if expect is not None else recs if ivs is None else rl.reduce_recs(recs, ivs)
    w5, w3, n_fwd, n_rev = cl.composition(kept, contigs, w, o)
    tot, (c5, c3), _ = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), w, q, ivs, **kw)
    assert np.array_equal(c5, w5), (w, kernel, "c5", c5.astype(np.int64) - w5.astype(np.int64))
    assert np.array_equal(c3, w3), (w, kernel, "c3", c3.astype(np.int64) - w3.astype(np.int64))
    n5, n3 = rows_exist(kept, contigs, w, o)
    assert np.array_equal(c5.sum(axis=1), n5) and np.array_equal(c3.sum(axis=1), n3)
    return tot, c5, c3, (n_fwd, n_rev)


# ---- 1. widths, lengths, region lengths, alignment, strands ---------------------------------------------------------------

def clean():
    text = il.clean_contig(9000, seed=61)
    return [("c", text)], [("c", len(text))], text


def spread_records(text: str, lengths=LENGTHS, rname: str = "c", tag: str = ""):
    """<L>M records of every length at every start mod 8 on both strands, with names of every length mod 4 (the record's
    offset in the block)"""
    recs, n = [], 0
    for L in lengths:
        for a in range(8):
            for flag in (0, 16):
                n += 1
                recs.append(il.read_on(text, 200 + 37 * n + (a - (200 + 37 * n)) % 8, L, name=f"{tag}e{n:03d}" + "x" * (n % 4), flag=flag, rname=rname))
    return recs


def test_spread_records_hold_what_they_claim():
    """(no GPU work)"""
    _, _, text = clean()
    recs = spread_records(text)
    for L in LENGTHS:
        mine = [r for r in recs if len(r.seq) == L]
        assert {(r.pos - 1) % 8 for r in mine if r.flag == 0} == set(range(8)) == {(r.pos - 1) % 8 for r in mine if r.flag == 16}
    assert {len(r.qname) % 4 for r in recs} == {0, 1, 2, 3}


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w", WIDTHS)
def test_widths_lengths_and_region_lengths(pkg, w, kernel):
    """reads shorter than the window: the inside offsets at and beyond L stay empty, and the two blocks overlap; under -r 30 the
    reads below 30 bases are filtered and count nothing"""
    contigs, refs, text = clean()
    recs = spread_records(text)
    for n in REGION_LENS:
        o = tl.PssOpts(region_len=n)
        tot, c5, c3, (n_fwd, n_rev) = check(pkg, contigs, refs, recs, o, kernel, w)
        entered = [r for r in recs if len(r.seq) >= n]
        assert n_fwd == n_rev == len(entered) == tot.stats["pss_ok"]
        for c in (c5, c3):
            assert int(c[w - 1].sum()) == len(entered)                                # the base next to the read always exists here
            for j in range(w):
                assert int(c[w + j].sum()) == sum(1 for r in entered if len(r.seq) > j)
            assert not c[:, 4].any()                                                  # a clean contig: nothing but A C G T


# ---- 2. letters, contig edges, the padding ---------------------------------------------------------------------------------

def odd_contig():
    odd = list(il.clean_contig(3000, seed=62))
    odd[1000:1100] = "".join(odd[1000:1100]).lower()                     # lower case: folded, counts like upper case
    for p in range(1200, 1400, 7):
        odd[p] = "N"
    for p in range(1203, 1400, 7):
        odd[p] = "RYKMSWBDHV"[p % 10]
    for p in range(1206, 1400, 14):
        odd[p] = "n"
    return "".join(odd)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w", [3, 30])
def test_other_letters_next_to_the_ends(pkg, w, kernel):
    odd = odd_contig()
    contigs, refs = [("odd", odd)], [("odd", len(odd))]
    recs = []
    for a in range(40):
        for flag in (0, 16):
            recs.append(il.read_on(odd, 1190 + 3 * a, 20 + a % 9, name=f"o{a}" + "x" * (a % 4), flag=flag, rname="odd"))
            recs.append(il.read_on(odd, 990 + 3 * a, 31, name=f"l{a}", flag=flag, rname="odd"))
    letters = cl.fasta_letters(contigs)
    for o in (tl.PssOpts(region_len=3), tl.PssOpts(region_len=3, up_ctx=letters, down_ctx=letters)):
        tot, c5, c3, (n_fwd, _) = check(pkg, contigs, refs, recs, o, kernel, w)
        assert int(c5[:, 4].sum()) > 20 and int(c3[:, 4].sum()) > 20                  # N and IUPAC letters are "other", on both strands
    assert n_fwd == len(recs)                                                         # with every letter in -U / -D nothing is rejected
    assert int(c5[w - 1, 4]) > 5 and int(c3[w - 1, 4]) > 5                            # ... the reads next to an N among them


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w", [3, 29, 30])
def test_contig_edges_and_the_neighbour(pkg, w, kernel):
    """two contigs that lie next to each other in the engine's genome: reads at s = 2 of the second and at s + L + 2 = len of
    the first.  The first contig ends in G's and the second starts with C's, the reads' own letters are A and T: an offset
    beyond the edge must count nothing, and no letter of the neighbour (or of the padding) may appear"""
    first = il.clean_contig(600, seed=63)[:500].replace("G", "A") + "A" * 40 + "GG"
    second = "CC" + "T" * 40 + il.clean_contig(600, seed=64)[:500].replace("C", "T")
    contigs = [("k1", first), ("k2", second)]
    refs = [(nm, len(t)) for nm, t in contigs]
    recs = []
    for L in (1, 5, 9, 31):
        for flag in (0, 16):
            recs.append(il.read_on(second, 2, L, name=f"s{L}", flag=flag, rname="k2"))
            recs.append(il.read_on(first, len(first) - L - 2, L, name=f"f{L}x", flag=flag, rname="k1"))
            for a in range(3, 11):                                                   # and a few bases further in, every start mod 8
                recs.append(il.read_on(second, a, L, name=f"t{L}{a}", flag=flag, rname="k2"))
                recs.append(il.read_on(first, len(first) - L - a, L, name=f"g{L}{a}", flag=flag, rname="k1"))
    o = tl.PssOpts(region_len=0)
    tot, c5, c3, (n_fwd, n_rev) = check(pkg, contigs, refs, recs, o, kernel, w)
    assert n_fwd == n_rev == len(recs)
    only = [r for r in recs if r.rname == "k2"]
    fwd_only = [r for r in only if not r.flag & 16]
    _, c5, _, _ = check(pkg, contigs, refs, fwd_only, o, kernel, w)
    assert int(c5[w - 1].sum()) == len(fwd_only) and int(c5[w - 2].sum()) == len(fwd_only)
    if w >= 3:
        assert int(c5[w - 3].sum()) == sum(1 for r in fwd_only if r.pos - 1 >= 3) < len(fwd_only)
    assert not c5[:w, 2].any() and not c5[:w, 0].any()                                 # no G of k1's end, no A: only k2's own C and T
    if w >= 11:
        assert not c5[:w - 10].any()                                                   # nothing starts more than 10 bases in
    last = [r for r in recs if r.rname == "k1" and not r.flag & 16]
    _, _, c3, _ = check(pkg, contigs, refs, last, o, kernel, w)
    assert not c3[:w, 1].any() and not c3[:w, 3].any()                                 # no C / T of k2's start behind k1's end: only A and G
    if w >= 11:
        assert not c3[:w - 10].any()


# ---- 3. mates, flags and every filter --------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_mates_and_flags(pkg, kernel):
    """a read 1 counts in the 5' block only, a read 2 in the 3' block only, an unpaired read in both; without the proper-pair flag
    or with the mate-unmapped flag a paired record counts nothing; the record with both mate flags is a read 1 where -U lets it,
    else a read 2"""
    contigs, refs, text = clean()
    L, w = 44, 8
    o = tl.PssOpts(region_len=5, up_ctx="A", down_ctx="C", min_mq=10)
    s_ok = next(p for p in range(100, 8000) if text[p - 1] == "A" and text[p + L] == "C")
    s_noU = next(p for p in range(100, 8000) if text[p - 1] != "A" and text[p + L] == "C")
    s_noD = next(p for p in range(100, 8000) if text[p - 1] == "A" and text[p + L] != "C")
    s_none = next(p for p in range(100, 8000) if text[p - 1] != "A" and text[p + L] != "C")
    P = 0x1 | 0x2
    groups = {
        "read1": ([il.read_on(text, s_ok, L, flag=P | 0x40, tlen=L)], (1, 0)),
        "read2": ([il.read_on(text, s_ok, L, flag=P | 0x80, tlen=-L)], (0, 1)),
        "read1_reverse": ([il.read_on(text, s_ok, L, flag=P | 0x40 | 0x10, tlen=-L)], None),
        "unpaired": ([il.read_on(text, s_ok, L)], (1, 1)),
        "read1_not_proper": ([il.read_on(text, s_ok, L, flag=0x1 | 0x40, tlen=L)], (0, 0)),
        "read2_mate_unmapped": ([il.read_on(text, s_ok, L, flag=P | 0x8 | 0x80, tlen=L)], (0, 0)),
        "both_mate_flags": ([il.read_on(text, s_ok, L, flag=P | 0xC0, tlen=L)], (1, 0)),
        "both_mate_flags_fails_U": ([il.read_on(text, s_noU, L, flag=P | 0xC0, tlen=L)], (0, 1)),
        "unpaired_fails_U": ([il.read_on(text, s_noU, L)], (0, 0)),
        "unpaired_fails_D": ([il.read_on(text, s_noD, L)], (0, 0)),
        "read1_fails_U": ([il.read_on(text, s_noU, L, flag=P | 0x40, tlen=L)], (0, 0)),
        "read2_fails_D": ([il.read_on(text, s_noD, L, flag=P | 0x80, tlen=L)], (0, 0)),
        "fails_both": ([il.read_on(text, s_none, L), il.read_on(text, s_none, L, flag=P | 0xC0, tlen=L)], (0, 0)),
        "reject_flags": ([il.read_on(text, s_ok, L, flag=f, name=f"f{f}") for f in (0x4, 0x100, 0x200, 0x400, 0x800)], (0, 0)),
        "low_mapq": ([il.read_on(text, s_ok, L, mapq=3)], (0, 0)),
        "cigar_not_one_match": ([replace(il.read_on(text, s_ok, L), cigar=[(L - 4, "M"), (4, "S")]), replace(il.read_on(text, s_ok, L), cigar=[(20, "M"), (2, "D"), (L - 20, "M")])], (0, 0)),
        "tlen_disagrees": ([il.read_on(text, s_ok, L, flag=P | 0x40, tlen=L + 3)], (0, 0)),
    }
    for name, (recs, n) in groups.items():
        tot, c5, c3, got = check(pkg, contigs, refs, recs, o, kernel, w)
        if n is not None:
            assert got == n, name
            assert int(c5.sum()) == n[0] * 2 * w and int(c3.sum()) == n[1] * 2 * w, name
    every = [r for recs, _ in groups.values() for r in recs]
    _, c5, c3, got = check(pkg, contigs, refs, every, o, kernel, w)
    assert got[0] >= 3 and got[1] >= 3


@pytest.mark.parametrize("kernel", KERNELS)
def test_length_merged_only_read_group_and_regions(pkg, kernel):
    """-l / -L, -m, -R and -T: a record they remove contributes nothing"""
    contigs, refs, text = clean()
    w = 5
    recs = [il.read_on(text, 300 + 90 * k, L, name=f"n{k}", flag=16 * (k & 1)) for k, L in enumerate((20, 30, 40, 50, 60, 70))]
    paired = [il.read_on(text, 1500 + 90 * k, 40, name=f"p{k}", flag=0x1 | 0x2 | (0x40 if k & 1 else 0x80), tlen=40) for k in range(4)]
    tot, c5, _, got = check(pkg, contigs, refs, recs + paired, tl.PssOpts(region_len=5, min_read_len=30, max_read_len=60), kernel, w)
    assert got == (4 + 2, 4 + 2) and tot.stats["pss_filtered"] == 2
    tot, _, _, got = check(pkg, contigs, refs, recs + paired, tl.PssOpts(region_len=5, merged_only=True), kernel, w)
    assert got == (6, 6) and tot.stats["pss_filtered"] == 4
    tagged = [replace(r, tags=[("RG", "Z", "grpA" if k % 3 else "grpB")]) for k, r in enumerate(recs + paired)]
    mine = [r for r in tagged if r.tags[0][2] == "grpA"]
    tot, _, _, got = check(pkg, contigs, refs, tagged + recs[:2], tl.PssOpts(region_len=5), kernel, w, expect=mine, read_group="grpA")
    assert 0 < got[0] < len(tagged) and tot.stats["rg_dropped"] == len(tagged) + 2 - len(mine)
    ivs = [("c", 330, 331), ("c", 700, 705), ("c", 1500, 1700)]                      # n0 (300..319) misses, n1 (390..419) misses, ...
    tot, _, _, got = check(pkg, contigs, refs, recs + paired, tl.PssOpts(region_len=5), kernel, w, ivs=ivs)
    kept = rl.reduce_recs(recs + paired, ivs)
    assert 0 < len(kept) < len(recs + paired) and tot.stats["pss_filtered"] == len(recs + paired) - len(kept)


# ---- 4. random records, the golden sets -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fuzz():
    return tl.fuzz_dataset(7511, 2000)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("w", [1, 10, 30])
@pytest.mark.parametrize("n", [0, 15, 30])
def test_random_records(pkg, fuzz, n, w, kernel):
    """tables, status counters and n_u64 - 20w are those of the engine without the setting"""
    contigs, refs, recs = fuzz
    o = tl.PssOpts(region_len=n)
    tot, c5, c3, (n_fwd, n_rev) = check(pkg, contigs, refs, recs, o, kernel, w)
    assert n_fwd > 200 and n_rev > 200 and c5[:, :4].all() and c3[:, :4].all()
    plain, _, n_plain = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), None)
    same_but_slow_path(tot, plain)
    if w >= 2:                                                                         # tie 1 on the engine's own tables
        assert cl.context_rows(tot.fwd, tot.rev) == {(b, -k): [int(x) for x in t[w - k, :4]] for b, t in (("c5", c5), ("c3", c3)) for k in (1, 2)}


@pytest.mark.parametrize("kernel", KERNELS)
def test_base_quality_changes_nothing(pkg, fuzz, kernel):
    contigs, refs, recs = fuzz
    o = tl.PssOpts(region_len=15)
    _, c5, c3, _ = check(pkg, contigs, refs, recs, o, kernel, 10)
    tq, q5, q3, _ = check(pkg, contigs, refs, recs, o, kernel, 10, q=20)
    assert np.array_equal(c5, q5) and np.array_equal(c3, q3)
    plain_q, _, _ = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), None, q=20)
    same_but_slow_path(tq, plain_q)


@pytest.mark.parametrize("kernel", KERNELS)
def test_regions_on_random_records(pkg, fuzz, kernel):
    contigs, refs, recs = fuzz
    ivs = rl.fuzz_intervals(7511, contigs, recs)
    o = tl.PssOpts(region_len=15)
    tot, c5, _, got = check(pkg, contigs, refs, recs, o, kernel, 10, ivs=ivs)
    whole = cl.composition(recs, contigs, 10, o)
    assert 0 < got[0] < whole[2] and tot.stats["pss_filtered"] > 0
    check(pkg, contigs, refs, recs, o, kernel, 10, q=20, ivs=ivs)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("base", ["setA", "setD"])
def test_golden_sets(pkg, base, kernel):
    """the three ties, on the engine: the rows the unmodified reference wrote"""
    contigs = sc.read_fasta(GOLD / f"{base}.fa")
    refs, recs = ml.read_sam(GOLD / f"{base}.sam")
    w, ties = cl.parse_golden((GOLD / f"composition10_{base}.txt").read_text())
    rows = lambda c5, c3, js: {(b, j): [int(x) for x in t[j + w, :4]] for b, t in (("c5", c5), ("c3", c3)) for j in js}   # noqa: E731
    _, c5, c3, _ = check(pkg, contigs, refs, recs, tl.PssOpts(), kernel, w)
    assert rows(c5, c3, (-1, -2)) == ties["tie1"]
    _, c5, c3, _ = check(pkg, contigs, refs, recs, tl.PssOpts(region_len=w), kernel, w)
    assert rows(c5, c3, range(w)) == ties["tie2"]
    letters = cl.fasta_letters(contigs)
    far = cl.far_from_edges(recs, contigs, w, 15)
    _, c5, c3, _ = check(pkg, contigs, refs, far, tl.PssOpts(up_ctx=letters, down_ctx=letters), kernel, w)
    assert rows(c5, c3, range(-w, -2)) == ties["tie3"]


# ---- 5. several tiles per workgroup, the one-lane path, wide counts, the compressed feed --------------------------------------

SHAPES = {
    "one_wg": {"PSSBAM_GRID_WGS": "1", "PSSBAM_TILE_READS": "48"},
    "three_wg": {"PSSBAM_GRID_WGS": "3", "PSSBAM_TILE_READS": "48"},
    "xcd8": {"PSSBAM_XCD_MAP": "1", "PSSBAM_GRID_WGS": "8", "PSSBAM_TILE_READS": "48"},
    "simple_one_block": {"PSSBAM_SIMPLE_BLOCKS": "1"},
}


@pytest.fixture(scope="module")
def seven_hundred():
    return tl.fuzz_dataset(9701, 700)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_several_tiles_per_workgroup(pkg, seven_hundred, monkeypatch, shape):
    """700 records in tiles of 48: the LDS words must survive the tile loop"""
    for key, v in SHAPES[shape].items():
        monkeypatch.setenv(key, v)
    kernel = "SIMPLE" if shape == "simple_one_block" else "TILED"
    for w in (3, 30):
        _, _, _, got = check(pkg, *seven_hundred, tl.PssOpts(region_len=15), kernel, w)
        assert got[0] > 80 and got[1] > 80


@pytest.fixture(scope="module")
def tiles():
    contigs, refs, recs = tl.fuzz_dataset(9601, 3200)
    assert_every_tile_overflows(tl.raw_records(refs, recs))      # with 5 pieces every tile of 64 holds an overflow record
    return contigs, refs, recs


@pytest.mark.parametrize("q", [0, 20])
def test_one_lane_path(pkg, tiles, monkeypatch, q):
    """records too long for the staged prefix go through count_composition inside the tiled kernel and add the same counts"""
    for key, v in {"PSSBAM_GRID_WGS": "2", "PSSBAM_TILE_READS": "64", "PSSBAM_PIECES": "5"}.items():
        monkeypatch.setenv(key, v)
    tot, _, _, got = check(pkg, *tiles, tl.PssOpts(region_len=15), "TILED", 10, q=q)
    assert got[0] > 500 and tot.stats["slow_path"] >= 50
    monkeypatch.delenv("PSSBAM_PIECES")
    fast, _, _, _ = check(pkg, *tiles, tl.PssOpts(region_len=15), "TILED", 10, q=q)
    same_but_slow_path(tot, fast)


@pytest.mark.parametrize("kernel", KERNELS)
def test_seventy_thousand_identical_records(pkg, kernel):
    """every word that is hit takes 70 000 (or 140 000) counts: more than 16 bits hold, from one position"""
    contigs, refs, text = clean()
    n, w = 70000, 30
    recs = [il.read_on(text, 1003, 33, name="same"), il.read_on(text, 1003, 33, name="same", flag=16)]
    block = np.tile(tl.raw_records(refs, recs), n // 2)
    o = tl.PssOpts(region_len=5)
    w5, w3, _, _ = cl.composition(recs, contigs, w, o)
    eng = pkg.Engine(pss=pss_dict(o), kernel=kern(pkg, kernel), composition=w)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(block)
    c5, c3 = eng.finish_composition()
    tot = eng.finish()
    eng.close()
    assert tot.stats["pss_ok"] == n
    assert np.array_equal(c5, w5 * np.uint64(n // 2)) and np.array_equal(c3, w3 * np.uint64(n // 2))
    assert int(c5.max()) >= n // 2 > 1 << 15 and int(c5.sum()) == 2 * w * n == int(c3.sum())


def test_one_workgroup_walks_more_than_8192_tiles(pkg, monkeypatch):
    """the LDS words are handed to the counter block every 8192 tiles of a workgroup (so that a u32 word cannot wrap): one
    workgroup, tiles of 16 reads, 8 200 tiles -- the counts on both sides of the hand-over add up"""
    monkeypatch.setenv("PSSBAM_GRID_WGS", "1")
    monkeypatch.setenv("PSSBAM_TILE_READS", "16")
    contigs, refs, text = clean()
    recs = [il.read_on(text, 100 + 13 * j, 24, name=f"t{j:03d}", flag=16 * (j & 1)) for j in range(160)]
    o, w, times = tl.PssOpts(region_len=5), 30, 820
    w5, w3, n_fwd, n_rev = cl.composition(recs, contigs, w, o)
    assert n_fwd == n_rev == 160 and w5[:w + 24, :4].all() and w3[:w + 24, :4].all() and not np.array_equal(w5, w3)
    assert int(w5[w + 23].sum()) == 160 and not w5[w + 24:].any()              # reads of 24 bases: the inside offsets from 24 on stay empty
    block = np.tile(tl.raw_records(refs, recs), times)
    eng = pkg.Engine(pss=pss_dict(o), kernel=pkg.KERNEL_TILED, composition=w)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(block)
    c5, c3 = eng.finish_composition()
    tot = eng.finish()
    eng.close()
    assert tot.stats["records"] == 160 * times > 8192 * 16 and tot.stats["pss_ok"] == 160 * times
    assert np.array_equal(c5, w5 * np.uint64(times)) and np.array_equal(c3, w3 * np.uint64(times))


def test_submit_bgzf(pkg, fuzz, tmp_path):
    """the compressed feed (device-indexed blocks) goes through the same launches; the setting follows feed_open"""
    contigs, refs, recs = fuzz
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    o = tl.PssOpts(region_len=15)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_composition(10)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    c5, c3 = eng.finish_composition()
    tot = eng.finish()
    assert eng.feed_status()["flags"] == 0
    eng.close()
    w5, w3, n_fwd, _ = cl.composition(recs, contigs, 10, o)
    assert np.array_equal(c5, w5) and np.array_equal(c3, w3) and tot.stats["records"] == len(recs) and n_fwd > 200


# ---- 6. off is off, reset, reduce, rules -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["AUTO", "SIMPLE", "TILED"])
def test_off_is_off(pkg, fuzz, kernel):
    contigs, refs, recs = fuzz
    o = tl.PssOpts(region_len=15)
    plain, _, n_plain = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), None)
    eng = pkg.Engine(pss=pss_dict(o), kernel=kern(pkg, kernel), composition=4)
    lay = eng.counter_layout()
    assert eng.counters_device()[1] == n_plain + 80 == lay["n_u64"] and lay["comp5"] == n_plain and lay["comp3"] == n_plain + 40
    eng.set_composition(30)                                 # another width before the first tally: the block follows
    assert eng.counters_device()[1] == n_plain + 600 == eng.counter_layout()["n_u64"]
    eng.set_composition(0)
    assert eng.composition is None and eng.counters_device()[1] == n_plain == eng.counter_layout()["n_u64"]
    assert "comp5" not in eng.counter_layout()
    with pytest.raises(pkg.PssbamError):
        eng.finish_composition()
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    tot = eng.finish()
    eng.close()
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev) and tot.stats == plain.stats
    on, (c5, c3), n_on = run_engine(pkg, contigs, refs, recs, o, kern(pkg, kernel), 4)     # on (AUTO included): tables and stats untouched
    assert n_on == n_plain + 80
    same_but_slow_path(on, plain)
    w5, w3, _, _ = cl.composition(recs, contigs, 4, o)
    assert np.array_equal(c5, w5) and np.array_equal(c3, w3)


def test_reset_keeps_the_setting_and_reduce_sums_the_words(pkg, fuzz):
    contigs, refs, recs = fuzz
    o = tl.PssOpts(region_len=15)
    w5, w3, _, _ = cl.composition(recs, contigs, 9, o)

    def make():
        eng = pkg.Engine(pss=pss_dict(o), composition=9)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        return eng

    eng = make()
    n = eng.counters_device()[1]
    eng.submit(tl.raw_records(refs, recs))
    with pytest.raises(pkg.PssbamError):                   # records have been tallied
        eng.set_composition(3)
    first = eng.finish_composition()
    eng.reset()
    assert eng.composition == 9 and eng.counters_device()[1] == n
    z5, z3 = eng.finish_composition()
    assert not z5.any() and not z3.any()
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_composition()
    assert np.array_equal(first[0], w5) and np.array_equal(again[0], w5) and np.array_equal(first[1], w3) and np.array_equal(again[1], w3)
    eng.close()

    half = len(recs) // 2
    engs = [make(), make()]
    engs[0].submit(tl.raw_records(refs, recs[:half]))
    engs[1].submit(tl.raw_records(refs, recs[half:]))
    arr = (C.c_void_p * 2)(engs[0]._h, engs[1]._h)
    assert pkg.hip_lib().pssbam_reduce_counters(arr, 2, 0) == 0
    c5, c3 = engs[0].finish_composition()
    for e in engs:
        e.close()
    assert np.array_equal(c5, w5) and np.array_equal(c3, w3)


def test_rules(pkg):
    E = pkg.PssbamError
    for bad in (31, -1, 1 << 20):
        with pytest.raises(E):
            pkg.Engine(pss=dict(region_len=5), composition=bad)
    with pytest.raises(E):                                  # nothing is added to a table on a k-mer engine
        pkg.Engine(kmer=dict(klen=4), composition=4)
    with pytest.raises(E):
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), composition=4)
    with pytest.raises(E):                                  # fate and window are those of the one pass that holds all rows
        pkg.Engine(pss=dict(region_len=31), composition=4)
    others = (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]}), dict(per_contig=True), dict(replicates=4),
              dict(length_hist=100), dict(site_context="cpg"), dict(end_condition=(1, 13, 13)), dict(gapped=True),
              dict(mismatches=(4, -1, 0)), dict(mismatches=(0, 2, 0)), dict(interior=3))
    for kw in others:
        eng = pkg.Engine(pss=dict(region_len=5), **kw)
        with pytest.raises(E, match="exclude each other"):
            eng.set_composition(4)
        assert eng.composition is None
        eng.set_composition(0)                              # switching off what is off is always legal
        eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), composition=1)
    for setter, args in ((eng.set_read_groups, (["a"],)), (eng.set_length_bins, ([30],)), (eng.set_contig_sets, ({"x": ["chrA"]},)),
                         (eng.set_per_contig, (True,)), (eng.set_replicates, (4,)), (eng.set_length_histogram, (100,)),
                         (eng.set_site_context, ("cpg",)), (eng.set_end_condition, (1, 13, 13)), (eng.set_gapped, (True,)),
                         (eng.set_mismatches, (4, -1, 0)), (eng.set_mismatches, (0, 2, 0)), (eng.set_interior, (3,))):
        with pytest.raises(E, match="and the composition table exclude each other"):
            setter(*args)
    assert eng.composition == 1
    eng.set_composition(0)
    eng.set_length_histogram(100)                           # off again: the others are legal
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=30), read_group="grpA", min_base_qual=10, composition=30)   # goes with -R, -Q and -r 30
    assert eng.composition == 30
    eng.close()
    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    dptr, n = other.counters_device()
    eng.bind_counters(dptr, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_composition(4)
    eng.close()
    other.close()


# ---- 7. the command line -------------------------------------------------------------------------------------------------------

def run_cli(pkg, fa, aln, prefix, *more, env=None):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), *more], capture_output=True, text=True,
                          env={**os.environ, **(env or {})}, timeout=300)


def test_cli_on_setD(pkg, tmp_path):
    """-P 10 on setD.bam: the composition file is the restatement's, printed; counts and rates files are byte-equal to the run
    without -P"""
    fa, aln = GOLD / "setD.fa", GOLD / "setD.bam"
    for tag, args in (("with", ["-P", "10"]), ("without", [])):
        (tmp_path / tag).mkdir()
        pr = run_cli(pkg, fa, aln, tmp_path / tag / "out", *args)
        assert pr.returncode == 0, pr.stderr
        assert pr.stderr.splitlines()[0].endswith(" -P 10") == bool(args)
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == ["out.pss.composition.txt", "out.pss.counts.txt", "out.pss.rates.txt"]
    assert sorted(p.name for p in (tmp_path / "without").iterdir()) == ["out.pss.counts.txt", "out.pss.rates.txt"]
    for kind in ("counts", "rates"):
        a, b = ((tmp_path / tag / f"out.pss.{kind}.txt").read_text().replace(f"{tag}/out", "X/out") for tag in ("with", "without"))
        assert a == b, kind
    contigs = sc.read_fasta(fa)
    _, recs = ml.read_sam(GOLD / "setD.sam")
    w5, w3, _, _ = cl.composition(recs, contigs, 10)
    text = (tmp_path / "with" / "out.pss.composition.txt").read_text()
    assert text == cl.file_text(str(fa), str(aln), 10, w5, w3)
    w, c5, c3, f5, f3 = cl.parse_composition_file(text)
    assert w == 10 and np.array_equal(c5, w5) and np.array_equal(c3, w3) and f5[9] == cl.fractions(w5[9])
    _, ties = cl.parse_golden((GOLD / "composition10_setD.txt").read_text())
    assert [int(x) for x in c5[9, :4]] == ties["tie1"][("c5", -1)] and [int(x) for x in c3[8, :4]] == ties["tie1"][("c3", -2)]


def test_cli_two_engines(pkg, fuzz, tmp_path):
    """-P 30 -Q 20 -T, one engine and two engines whose counter blocks are summed: the same three files"""
    contigs, refs, recs = fuzz
    recs = [replace(r, qname=f"{r.qname}.{j}") for j in range(4) for r in tl.ref_safe(recs)]     # a few batches of 1 MiB
    fa, aln, bed = tmp_path / "g.fa", tmp_path / "in.bam", tmp_path / "t.bed"
    tl.write_fasta(fa, contigs)
    tl.write_bam(aln, refs, recs, rng=np.random.default_rng(2))
    ivs = rl.fuzz_intervals(7511, contigs, recs)
    rl.write_bed(bed, ivs)
    outs = {}
    for tag, e in (("one", {}), ("two", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"})):
        pr = run_cli(pkg, fa, aln, tmp_path / "out", "-P", "30", "-Q", "20", "-T", str(bed), env=e)
        assert pr.returncode == 0, pr.stderr
        outs[tag] = {kind: (tmp_path / f"out.pss.{kind}.txt").read_bytes() for kind in ("counts", "rates", "composition")}
    assert outs["one"] == outs["two"]
    w, c5, c3, _, _ = cl.parse_composition_file(outs["one"]["composition"].decode())
    w5, w3, n_fwd, _ = cl.composition(rl.reduce_recs(recs, ivs), contigs, 30, tl.PssOpts())
    assert w == 30 and np.array_equal(c5, w5) and np.array_equal(c3, w3) and n_fwd > 100

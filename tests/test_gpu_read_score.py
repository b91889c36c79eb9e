"""pss-bam -y / -Y on the GPU: a weighted score over the C and G sites of a whole read as a record filter and as a
histogram, summed in the tally kernels (tally_tiled's SCORE arm; tally_simple and the tiled kernel's one-lane path through
read_score).  The yardstick is the CPU oracle on reduced inputs built by read_score_lib:

    filter t:     fwd, rev and PSS_OK == the oracle's on the input without the <L>M records whose S is below t; every other
                  status slot and PSS_OK + PSS_FILTERED as the engine without the setting;
    histogram:    with OK(b) the oracle's PSS_OK on the records whose bin is b, per flag class as the mismatch histogram's
                  tests have it -- unpaired sf[b] == sr[b] == OK(b), first mates sf only, second mates sr only, any input
                  sf[b] + sr[b] == 2 * OK_unpaired(b) + OK_paired(b); tables and stats untouched.

Bit-exact (integer work).  test_read_score_host.py asserts without a GPU that no comparison here is vacuous."""
import ctypes as C
import os
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import pssbam_testlib as tl
import read_score_lib as rs
import regions_lib as rl
from test_gpu_length_hist import CLASSES, pss_dict, same_but_slow_path, split_by_flag
from test_gpu_tile_loop import assert_every_tile_overflows

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
KERNELS = ["SIMPLE", "TILED"]
OTHER_SLOTS = ("records", "rg_dropped", "parse_skip", "no_contig")
TABLES = rs.tables()


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def kern(pkg, name):
    return {"SIMPLE": pkg.KERNEL_SIMPLE, "TILED": pkg.KERNEL_TILED, "AUTO": pkg.KERNEL_AUTO}[name]


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, score=None, regions=None, **kw):
    """score: dict(weights=, min_score=, hist_half=, hist_shift=) or None -> (totals, (sf, sr) or None, n_u64)"""
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_score=score, **kw)
    assert (eng.read_score is None) == (score is None)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if regions is not None:
        eng.set_regions(*rl.to_arrays(regions))
    if recs:
        eng.submit(tl.raw_records(refs, recs))
    half = score.get("hist_half", 0) if score else 0
    hist = eng.finish_read_score() if half else None
    tot = eng.finish()
    n_u64 = eng.counters_device()[1]
    eng.close()
    if hist is not None:
        assert hist[0].shape == hist[1].shape == (2 * half,) and hist[0].dtype == np.uint64
    return tot, hist, n_u64


class Case:
    """a record set, its oracle genome, and memoised engine runs without the setting / oracle runs on reduced inputs"""

    def __init__(self, oracle, tmp: Path, contigs, refs, recs):
        self.oracle, self.tmp, self.contigs, self.refs, self.recs = oracle, tmp, contigs, refs, recs
        self.ctg = dict(contigs)
        self.g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
        self._plain, self._orc, self._rows, self._n = {}, {}, {}, 0

    def close(self):
        self.oracle.free_genome(self.g)

    def oracle_on(self, recs, o: tl.PssOpts):
        self._n += 1
        sam = self.tmp / f"o{self._n}.sam"
        tl.write_sam(sam, self.refs, recs)
        return self.oracle.pss(self.g, sam, o)

    def reduced(self, table: str, t: int, o: tl.PssOpts, q: int = 0, ivs=None):
        """the oracle on the input without the records below t -- S taken under the mask at base quality q, as defined; the
        kept records masked and reduced to the regions, where given"""
        key = (table, t, o.region_len, q, ivs is not None)
        if key not in self._orc:
            recs = rs.reduce_to(self.recs, self.ctg, TABLES[table], t, q)
            if q:
                recs = bq.mask_recs(recs, q)
            if ivs is not None:
                recs = rl.reduce_recs(recs, ivs)
            self._orc[key] = self.oracle_on(recs, o)
        return self._orc[key]

    def plain(self, pkg, o: tl.PssOpts, kernel: str, q: int = 0, ivs=None):
        """the totals of the engine without the setting"""
        key = (o.region_len, kernel, q, ivs is not None)
        if key not in self._plain:
            self._plain[key] = run_engine(pkg, self.contigs, self.refs, self.recs, o, kern(pkg, kernel), None, ivs, min_base_qual=q)[0]
        return self._plain[key]

    def ok_rows(self, o: tl.PssOpts, table: str, half: int, shift: int) -> dict:
        """{flag class: OK(b) for every bin b} from the oracle on every (class, bin) subset that holds a record"""
        key = (o.region_len, table, half, shift)
        if key not in self._rows:
            rows = {}
            for c, part in split_by_flag(self.recs).items():
                rows[c] = np.zeros(2 * half, dtype=np.uint64)
                for b, sub in enumerate(rs.split_by_bin(part, self.ctg, TABLES[table], half, shift)):
                    if sub:
                        rows[c][b] = self.oracle_on(sub, o)[2][tl.ST_OK]
            self._rows[key] = rows
        return self._rows[key]


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    case = Case(oracle, tmp_path_factory.mktemp("score"), *tl.fuzz_dataset(*rs.FUZZ))
    yield case
    case.close()


def setting(table: str, t=None, half: int = 0, shift: int = 0) -> dict:
    return dict(weights=TABLES[table], min_score=t, hist_half=half, hist_shift=shift)


def check_filter(pkg, case: Case, o, kernel: str, table: str, t: int, q: int = 0, ivs=None, half: int = 0, shift: int = 0):
    """one engine run with the filter against the oracle on the reduced input and the engine without the setting"""
    wf, wr, wst = case.reduced(table, t, o, q, ivs)
    plain = case.plain(pkg, o, kernel, q, ivs)
    tot, hist, _ = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), setting(table, t, half, shift), ivs, min_base_qual=q)
    assert np.array_equal(tot.fwd, wf) and np.array_equal(tot.rev, wr), (table, t, o.region_len, kernel)
    assert tot.stats["pss_ok"] == int(wst[tl.ST_OK])
    for slot in OTHER_SLOTS:
        assert tot.stats[slot] == plain.stats[slot], slot
    assert tot.stats["pss_ok"] + tot.stats["pss_filtered"] == plain.stats["pss_ok"] + plain.stats["pss_filtered"]
    return tot, hist, plain


# ---- 1. filter parity ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [0, 15, 30])
@pytest.mark.parametrize("table,t", [(name, t) for name, q, t in rs.CUTS if q == 0])
def test_filter_parity(pkg, fuzz, table, t, n, kernel):
    tot, _, plain = check_filter(pkg, fuzz, tl.PssOpts(region_len=n), kernel, table, t)
    assert 0 < tot.stats["pss_ok"] < plain.stats["pss_ok"]              # the filter bites and leaves something


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_with_min_base_quality(pkg, fuzz, kernel):
    """-Q takes positions out of S as it takes them out of the tables: S under the mask decides, the kept records are masked"""
    (table, q, t), = [c for c in rs.CUTS if c[1]]
    o = tl.PssOpts(region_len=15)
    tot, _, plain = check_filter(pkg, fuzz, o, kernel, table, t, q=q)
    assert not np.array_equal(plain.fwd, fuzz.plain(pkg, o, kernel).fwd)    # the mask did bite
    assert 0 < tot.stats["pss_ok"] < plain.stats["pss_ok"]
    unmasked = fuzz.reduced(table, t, o)
    assert tot.stats["pss_ok"] != int(unmasked[2][tl.ST_OK])               # and it moved reads across the threshold


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_with_regions(pkg, fuzz, kernel):
    ivs = rl.fuzz_intervals(7301, fuzz.contigs, fuzz.recs)
    o = tl.PssOpts(region_len=15)
    tot, _, plain = check_filter(pkg, fuzz, o, kernel, "pmd", -100, ivs=ivs)
    assert 0 < tot.stats["pss_ok"] < plain.stats["pss_ok"] < fuzz.plain(pkg, o, kernel).stats["pss_ok"]


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_with_min_base_quality_and_regions(pkg, fuzz, kernel):
    """the fourth instantiation of tally_tiled's SCORE arm: -Q and -T together"""
    (table, q, t), = [c for c in rs.CUTS if c[1]]
    ivs = rl.fuzz_intervals(7301, fuzz.contigs, fuzz.recs)
    o = tl.PssOpts(region_len=15)
    tot, _, plain = check_filter(pkg, fuzz, o, kernel, table, t, q=q, ivs=ivs)
    assert 0 < tot.stats["pss_ok"] < plain.stats["pss_ok"]


# ---- 2. histogram identities -----------------------------------------------------------------------------------------

def check_identities(pkg, case: Case, o, kernel: str, table: str, half: int, shift: int, t=None):
    """the per-class identities on the engine run over each subset, the sum identity on the run over all records, and
    tables + stats against an engine with the same filter and no histogram; bins below the filter's must be zero"""
    want = {c: v.copy() for c, v in case.ok_rows(o, table, half, shift).items()}
    first_kept = 0 if t is None else rs.score_bin(t, half, shift)
    if t is not None:
        assert t % (1 << shift) == 0                                   # the threshold lies on a bin edge: whole bins are cut
        for v in want.values():
            v[:first_kept] = 0
    zero = np.zeros(2 * half, dtype=np.uint64)
    parts = split_by_flag(case.recs)
    s = setting(table, t, half, shift)
    for c in CLASSES:
        _, (sf, sr), _ = run_engine(pkg, case.contigs, case.refs, parts[c], o, kern(pkg, kernel), s)
        if c == "unpaired":
            assert np.array_equal(sf, want[c]) and np.array_equal(sr, want[c]), (c, np.flatnonzero(sf != want[c]), np.flatnonzero(sr != want[c]))
        elif c == "first":
            assert np.array_equal(sf, want[c]) and np.array_equal(sr, zero), c
        elif c == "second":
            assert np.array_equal(sr, want[c]) and np.array_equal(sf, zero), c
        else:
            assert np.array_equal(sf + sr, want[c]), c
    tot, (sf, sr), n_u64 = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), s)
    paired = want["first"] + want["second"] + want["other"]
    assert np.array_equal(sf + sr, 2 * want["unpaired"] + paired)
    assert (sf >= want["unpaired"] + want["first"]).all() and (sr >= want["unpaired"] + want["second"]).all()
    if t is not None:
        assert not sf[:first_kept].any() and not sr[:first_kept].any()
        same, _, n_plain = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), setting(table, t))
    else:
        same, n_plain = case.plain(pkg, o, kernel), None
    same_but_slow_path(tot, same)
    assert int(sf.sum()) + int(sr.sum()) == 2 * tot.stats["pss_ok"] - int(paired.sum())   # an unpaired read counts in both arrays
    if n_plain is not None:
        assert n_u64 == n_plain + 4 * half
    return sf, sr, tot


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("table,half,shift", rs.HIST_SHAPES)
def test_histogram_identities(pkg, fuzz, table, half, shift, kernel):
    sf, sr, _ = check_identities(pkg, fuzz, tl.PssOpts(region_len=15), kernel, table, half, shift)
    assert sf[:half].any() and sf[half:].any() and sr[:half].any() and not np.array_equal(sf, sr)   # negative and positive scores
    if shift == 0 or half == 2:
        assert sf[0] + sr[0] > 0 and sf[-1] + sr[-1] > 0                                          # both clamps


@pytest.mark.parametrize("kernel", KERNELS)
def test_histogram_with_the_filter(pkg, fuzz, kernel):
    check_identities(pkg, fuzz, tl.PssOpts(region_len=15), kernel, "pmd", 2, 8, t=-256)
    check_identities(pkg, fuzz, tl.PssOpts(region_len=15), kernel, "wide", 128, 8, t=2048)


# ---- 3. random weight tables -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("table,t", [("wide", 0), ("narrow", -1500)])
def test_random_weight_table(pkg, fuzz, table, t, kernel):
    """the widest table [4][64][64] and the narrowest [4][1][1] in +-2047: every kind, both distance ends and the strand flip
    carry a weight of their own, and the kernel's sum is checked against read_score_lib's -- per read, through 256 bins of 64
    units (what is swapped or left out moves a read to another bin) and through the filter"""
    assert TABLES[table].shape == ((4, 64, 64) if table == "wide" else (4, 1, 1)) and np.abs(TABLES[table].astype(int)).max() <= 2047
    o = tl.PssOpts(region_len=15)
    sf, sr, _ = check_identities(pkg, fuzz, o, kernel, table, 128, 6)
    assert (sf > 0).sum() >= 40
    check_filter(pkg, fuzz, o, kernel, table, t)


# ---- 4. off is off, rules ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS + ["AUTO"])
def test_off_is_off(pkg, fuzz, kernel):
    o = tl.PssOpts(region_len=15)
    plain = fuzz.plain(pkg, o, kernel)
    eng = pkg.Engine(pss=pss_dict(o), kernel=kern(pkg, kernel))
    n_plain = eng.counters_device()[1]
    eng.set_read_score(TABLES["pmd"], min_score=0, hist_half=32, hist_shift=8)
    assert eng.counters_device()[1] == n_plain + 128 == eng.counter_layout()["n_u64"]
    assert eng.counter_layout()["score_fwd"] == n_plain and eng.counter_layout()["score_rev"] == n_plain + 64
    eng.set_read_score(None)
    assert eng.read_score is None and eng.counters_device()[1] == n_plain == eng.counter_layout()["n_u64"]
    with pytest.raises(pkg.PssbamError):
        eng.finish_read_score()
    eng.set_genome_arrays(tl.loaded_contigs(fuzz.contigs))
    eng.set_references([nm for nm, _ in fuzz.refs])
    eng.submit(tl.raw_records(fuzz.refs, fuzz.recs))
    tot = eng.finish()
    eng.close()
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev) and tot.stats == plain.stats
    # a minimum no read of the set falls below: the filter alone adds no words and drops nothing
    low, _, n_low = run_engine(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, kern(pkg, kernel), setting("pmd", -(2 ** 31)))
    assert n_low == n_plain
    same_but_slow_path(low, plain)


def test_rules(pkg):
    E = pkg.PssbamError
    W = TABLES["pmd"]
    ok = dict(weights=W, min_score=0, hist_half=4, hist_shift=8)
    bad_w = W.copy()
    bad_w[2, 5, 7] = 2048
    worse_w = W.copy()
    worse_w[0, 0, 0] = -2048
    for bad in (dict(ok, weights=np.zeros((4, 65, 2))), dict(ok, weights=np.zeros((4, 2, 65))), dict(ok, weights=np.zeros((4, 0, 2))),
                dict(ok, weights=np.zeros((4, 2, 0))), dict(ok, hist_half=129), dict(ok, hist_half=-1), dict(ok, hist_shift=17),
                dict(ok, hist_shift=-1), dict(ok, weights=bad_w), dict(ok, weights=worse_w), dict(ok, weights=np.zeros((3, 2, 2)))):
        with pytest.raises(E):
            pkg.Engine(pss=dict(region_len=5), read_score=bad)
    pkg.Engine(pss=dict(region_len=5), read_score=dict(ok, weights=np.full((4, 64, 64), -2047), hist_half=128, hist_shift=16)).close()
    with pytest.raises(E):                                  # nothing is added to a table on a k-mer engine
        pkg.Engine(kmer=dict(klen=4), read_score=ok)
    with pytest.raises(E):
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), read_score=ok)
    with pytest.raises(E):                                  # the decision is taken in the one pass that holds all rows
        pkg.Engine(pss=dict(region_len=31), read_score=ok)
    pkg.Engine(pss=dict(region_len=30), read_score=ok).close()
    others = (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]}), dict(per_contig=True), dict(replicates=4),
              dict(length_hist=100), dict(site_context="cpg"), dict(end_condition=(1, 13, 13)), dict(gapped=True), dict(mismatches=(4, 1, 0)),
              dict(mismatches=(0, 2, 0)), dict(interior=3), dict(composition=5))
    for kw in others:
        eng = pkg.Engine(pss=dict(region_len=5), **kw)
        for s in (ok, dict(ok, hist_half=0), dict(ok, min_score=None)):
            with pytest.raises(E):
                eng.set_read_score(**s)
        assert eng.read_score is None
        eng.set_read_score(None)                            # switching off what is off is always legal
        eng.close()
    for s in (dict(ok, hist_half=0), dict(ok, min_score=None)):
        eng = pkg.Engine(pss=dict(region_len=5), read_score=s)
        for setter, args in ((eng.set_read_groups, (["a"],)), (eng.set_length_bins, ([30],)), (eng.set_contig_sets, ({"x": ["chrA"]},)),
                             (eng.set_per_contig, (True,)), (eng.set_replicates, (4,)), (eng.set_length_histogram, (100,)),
                             (eng.set_site_context, ("cpg",)), (eng.set_end_condition, (1, 13, 13)), (eng.set_gapped, (True,)),
                             (eng.set_mismatches, (4, -1, 0)), (eng.set_mismatches, (0, 1, 0)), (eng.set_interior, (3,)), (eng.set_composition, (5,))):
            with pytest.raises(E):
                setter(*args)
        assert eng.read_score is not None and eng.read_score["hist_half"] == s["hist_half"]
        eng.set_read_score(None)
        eng.set_length_histogram(100)                       # off again: the others are legal
        eng.close()

    eng = pkg.Engine(pss=dict(region_len=5), read_group="grpA", min_base_qual=10, read_score=ok)   # goes with -R and -Q
    lay = eng.counter_layout()
    assert lay["score_fwd"] == lay["stats"] + pkg.ST_N and lay["score_rev"] == lay["score_fwd"] + 8
    assert lay["n_u64"] == lay["score_rev"] + 8 == eng.counters_device()[1]
    contigs, refs, recs = tl.fuzz_dataset(5, 300, with_rg=True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    for s in (None, ok, dict(ok, hist_half=0)):
        with pytest.raises(E):                              # records have been tallied
            eng.set_read_score(**(s or dict(weights=None)))
    first = eng.finish_read_score()
    assert first[0].sum() > 0
    eng.reset()                                             # the setting survives reset
    assert eng.counters_device()[1] == lay["n_u64"]
    zf, zr = eng.finish_read_score()
    assert not zf.any() and not zr.any()
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_read_score()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    eng.reset()
    eng.set_read_score(**dict(ok, hist_half=2))             # legal again after reset
    assert eng.counters_device()[1] == eng.counter_layout()["n_u64"] == lay["score_fwd"] + 8
    eng.close()

    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_read_score(**ok)
    eng.set_read_score(**dict(ok, hist_half=0))             # the filter alone adds no words
    assert eng.counters_device() == (d, n)
    eng.close()
    other.close()


# ---- 5. edges ----------------------------------------------------------------------------------------------------------

EDGE_LENGTHS = (1, 7, 8, 9, 16, 17, 33, 150)
EDGE_TABLES = {"small": np.random.default_rng(5).integers(-4, 5, size=(4, 6, 64)).astype(np.int16),          # exact at shift 0: |S| stays below 128
               "large": np.random.default_rng(6).integers(-2047, 2048, size=(4, 6, 64)).astype(np.int16)}    # bins of 64 units
TABLES.update({f"edge_{k}": v for k, v in EDGE_TABLES.items()})
EDGE_RUNS = (("edge_small", 0), ("edge_large", 6))


def sparse_contig(n: int, seed: int) -> str:
    """A / T at random with a C at every tenth position and a G five behind it: a read holds a site every five bases, whose
    distances from its ends are set by where it starts"""
    rng = np.random.default_rng(seed)
    t = ["AT"[int(x)] for x in rng.integers(0, 2, size=n)]
    for p in range(0, n, 10):
        t[p] = "C"
    for p in range(5, n, 10):
        t[p] = "G"
    return "".join(t)


def edge_contigs():
    fwd = sparse_contig(4000, 31)
    odd = list(sparse_contig(2000, 32))
    odd[500:600] = "".join(odd[500:600]).lower()                         # lower case: folded, scores like upper case
    for p in range(1000, 1100, 20):                                      # N and Y where a C would be, R where a G would be
        odd[p] = "N"
        odd[p + 10] = "Y"
        odd[p + 5] = "R"
    return [("c", fwd), ("rc", rs.revcomp(fwd)), ("odd", "".join(odd))]


def damaged(ctg: str, s: int, L: int, which: str, **kw) -> tl.Rec:
    """the read at s that copies the contig but for: "" nothing, "ct" every C read as T, "ga" every G read as A, "both", "n" an N on
    the first and last site, "iupac" a Y / R on them, "other" every C read as A and every G read as T (adds nothing)"""
    sites = [i for i in range(L) if ctg[s + i].upper() in "CG"]
    subs = {}
    for i in sites:
        b = ctg[s + i].upper()
        if which in ("ct", "both") and b == "C":
            subs[i] = "T"
        if which in ("ga", "both") and b == "G":
            subs[i] = "A"
        if which == "other":
            subs[i] = "A" if b == "C" else "T"
    if which in ("n", "iupac") and sites:
        for i in (sites[0], sites[-1]):
            subs[i] = "N" if which == "n" else ("Y" if ctg[s + i].upper() == "C" else "R")
    return rs.read_on(ctg, s, L, subs, **kw)


def edge_groups():
    """{name: (region_len, [records])}"""
    (_, fwd), (_, rc), (_, odd) = edge_contigs()
    G, n = {}, [0]

    def name():                                                            # read names of every length mod 4: the record's offset in the block
        n[0] += 1
        return f"e{n[0]:04d}" + "x" * (n[0] % 4)

    # every length around the half cut (a multiple of 8), at every start mod 10: sites at i and L-1-i = 4, 5, 6 = n_dist-2 .. n_dist
    lengths, twins = [], []
    for L in EDGE_LENGTHS:
        for a in range(10):
            s = 100 + 20 * L + a
            for which in ("", "ct", "ga", "both"):
                r = damaged(fwd, s, L, which, name=name())
                lengths.append(r)
                twins.append(rs.revcomp_twin(r, "rc", len(fwd) - s - L))    # reverse-strand twin on the reverse-complemented contig
                lengths.append(replace(r, qname=name(), flag=16))        # and the same read called reverse: the kinds swap
    G["lengths"] = (0, lengths)
    G["twins"] = (0, twins)
    quiet = []
    for a in range(10):
        s = 1500 + 70 * a + a
        quiet += [damaged(fwd, s, 60, w, name=name()) for w in ("n", "iupac", "other")]
        quiet += [damaged(odd, 990 + a, 120, w, name=name(), rname="odd") for w in ("", "both")]              # N, Y, R in the reference
        quiet += [damaged(odd, 490 + a, 120, w, name=name(), rname="odd") for w in ("", "ct", "ga")]          # lower case in the reference
    G["non_counting"] = (5, quiet)
    quals = []
    for a in range(10):
        s, L = 2500 + 50 * a + a, 40
        for w in ("", "both"):
            r = damaged(fwd, s, L, w, name=name())
            for v in (0, 19, 20, 62, 63, 64, 93):
                quals.append(rs.with_qual(replace(r, qname=name()), [v if i % 5 == (-s) % 5 else (i * 7) % 94 for i in range(L)]))
    G["qualities"] = (5, quals)
    # QUAL 0xFF (absent: the last column, and never below a minimum): only a read of one base is tallied without qualities
    G["absent_qual"] = (0, [rs.with_qual(damaged(fwd, 3300 + 5 * k, 1, w, name=name(), flag=fl), q) for k in range(8) for w in ("", "both")
                            for fl in (0, 16) for q in ("*", [0], [40])])
    flags = []
    for a in range(10):
        s, L = 3000 + 60 * a + a, 44
        for fl, tlen in ((0x1 | 0x2 | 0x40, L), (0x1 | 0x2 | 0x80, -L), (0x1 | 0x2 | 0x40 | 0x10, -L), (0x1 | 0x2 | 0x80 | 0x10, L)):
            flags += [damaged(fwd, s, L, w, name=name(), flag=fl, tlen=tlen) for w in ("", "both")]
        # l_seq < L and l_seq > L: a mate whose |TLEN| and CIGAR say 44 and whose SEQ holds 31, 40 or 50 bases
        for n_seq in (31, 40, 50):
            flags += [rs.read_on(fwd, s, L, {i: "T" for i in range(n_seq) if fwd[s + i] == "C"}, name=name(), flag=0x1 | 0x2 | 0x40, tlen=L, seq_len=n_seq)]
    G["flags_and_lengths"] = (5, flags)
    # hanging over either contig end (never a candidate: no context bases there), and the last reads that are
    ends = [rs.read_on(fwd, len(fwd) - 10, 30, name=name()), rs.read_on(fwd, len(fwd) - 31, 30, name=name()), rs.read_on(fwd, len(fwd) - 32, 30, name=name()),
            rs.read_on(fwd, 0, 30, name=name()), rs.read_on(fwd, 1, 30, name=name()), rs.read_on(fwd, 2, 30, name=name()),
            replace(rs.read_on(fwd, 0, 30, name=name()), pos=0)]
    G["contig_ends"] = (5, ends)
    return G


@pytest.fixture(scope="module")
def edges(oracle, tmp_path_factory):
    contigs = edge_contigs()
    refs = [(nm, len(s)) for nm, s in contigs]
    cases = {nm: (n, Case(oracle, tmp_path_factory.mktemp(f"sedge_{nm}"), contigs, refs, recs)) for nm, (n, recs) in edge_groups().items()}
    yield cases
    for _, c in cases.values():
        c.close()


def added_to(case: Case, o) -> list:
    """[(in the forward table, in the reverse table)] per record, by the plain oracle: one run per record, once"""
    if not hasattr(case, "added"):
        case.added = [tuple(int(x.any()) for x in case.oracle_on([r], o)[:2]) for r in case.recs]
    return case.added


def edge_expectation(case: Case, o, table: str, shift: int, q: int = 0):
    """(sf, sr) straight from read_score_lib: a record the plain oracle adds to a table counts in its bin"""
    added_to(case, o)
    sf, sr = np.zeros(256, dtype=np.uint64), np.zeros(256, dtype=np.uint64)
    for r, (in_f, in_r) in zip(case.recs, case.added):
        b = rs.score_bin(rs.score(r, case.ctg, TABLES[table], q), 128, shift)
        sf[b] += in_f
        sr[b] += in_r
    return sf, sr


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("group", ["lengths", "twins", "non_counting", "qualities", "absent_qual", "flags_and_lengths", "contig_ends"])
def test_edges(pkg, edges, group, kernel):
    n, case = edges[group]
    o = tl.PssOpts(region_len=n)
    added = [bool(f or r) for f, r in added_to(case, o)]            # (every record but those over a contig end and with l_seq > L)
    assert sum(added) == len(case.recs) or group in ("contig_ends", "flags_and_lengths")
    for table, shift in EDGE_RUNS:
        for q in ((0, 20) if group in ("qualities", "absent_qual") else (0,)):
            want_f, want_r = edge_expectation(case, o, table, shift, q)
            tot, (sf, sr), _ = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), setting(table, None, 128, shift), min_base_qual=q)
            assert np.array_equal(sf, want_f) and np.array_equal(sr, want_r), (table, q, np.flatnonzero(sf != want_f), np.flatnonzero(sr != want_r))
            same_but_slow_path(tot, case.plain(pkg, o, kernel, q))
            assert tot.stats["pss_ok"] == sum(added)
            if group != "contig_ends":
                assert sum(added) >= 0.8 * len(case.recs) and (sf > 0).sum() + (sr > 0).sum() >= 6
    scores = sorted(rs.score(r, case.ctg, TABLES["edge_large"]) for r, a in zip(case.recs, added) if a)
    t = scores[len(scores) // 2]
    ftot, _, _ = check_filter(pkg, case, o, kernel, "edge_large", t)
    assert ftot.stats["pss_ok"] == sum(s >= t for s in scores)


def test_edge_groups_hold_what_they_claim():
    """(no GPU work) the hand-built records against the definition"""
    G = edge_groups()
    ctg = dict(edge_contigs())
    W = EDGE_TABLES["small"]
    S = lambda r, q=0: rs.score(r, ctg, W, q)      # noqa: E731
    assert all(S(r) is not None for _, recs in G.values() for r in recs)
    assert max(abs(S(r)) for _, recs in G.values() for r in recs) < 128                               # shift 0 tells every score apart
    lengths, twins = G["lengths"][1], G["twins"][1]
    assert {len(r.seq) for r in lengths} == set(EDGE_LENGTHS) and {(r.pos - 1) % 10 for r in lengths} == set(range(10))
    assert {len(r.qname) % 4 for r in lengths} == {0, 1, 2, 3}
    fw = [r for r in lengths if not r.flag & 16]
    assert len(fw) == len(twins) and all(t.flag & 16 for t in twins)
    assert [S(r) for r in fw] == [S(t) for t in twins]                                                # the twin's score is the read's
    assert [rs.score(r, ctg, EDGE_TABLES["large"]) for r in fw] == [rs.score(t, ctg, EDGE_TABLES["large"]) for t in twins]
    assert sum(S(r) != S(replace(r, flag=16)) for r in fw) > len(fw) // 2                               # the strand flag alone changes it
    # sites at distance n_dist - 2, n_dist - 1 and n_dist from either end, on reads long enough to have them
    for r in (r for r in fw if len(r.seq) >= 16):
        s, L = r.pos - 1, len(r.seq)
        assert {(-s) % 10, (5 - s) % 10} == {i % 10 for i in range(L) if ctg["c"][s + i] in "CG"} and L
    assert {(-(r.pos - 1)) % 10 for r in fw} >= {4, 5, 6} and {(len(r.seq) - 1 - ((5 - (r.pos - 1)) % 10)) % 10 for r in fw} >= {4, 5, 6}
    quiet = G["non_counting"][1]
    assert S(quiet[2]) == 0 and S(quiet[0]) != S(rs.read_on(ctg["c"], quiet[0].pos - 1, 60))          # "other" adds nothing; an N takes a site out
    quals = G["qualities"][1]
    assert {q for r in quals for q in rs.qual_bytes(r)} >= {0, 19, 20, 62, 63, 64, 93}
    assert any(S(r) != S(r, 20) for r in quals)
    absent = G["absent_qual"][1]
    assert {r.qual for r in absent} == {"*", "!", "I"} and all(len(r.seq) == 1 and ctg["c"][r.pos - 1] in "CG" for r in absent)
    L = lambda r, q=0: rs.score(r, ctg, EDGE_TABLES["large"], q)      # noqa: E731
    assert any(L(r) != L(r, 20) for r in absent if r.qual == "!") and all(L(r) == L(r, 93) != 0 for r in absent if r.qual == "*")
    assert len({L(r) for r in absent}) >= 12                                                          # kind and column tell apart
    fl = G["flags_and_lengths"][1]
    assert {len(r.seq) - abs(r.tlen) for r in fl if r.flag & 1} == {0, -13, -4, 6}


# ---- 6. several tiles per workgroup and the one-lane path -------------------------------------------------------------

SHAPES = {
    "one_wg": {"PSSBAM_GRID_WGS": "1", "PSSBAM_TILE_READS": "48"},
    "three_wg": {"PSSBAM_GRID_WGS": "3", "PSSBAM_TILE_READS": "48"},
    "xcd8": {"PSSBAM_XCD_MAP": "1", "PSSBAM_GRID_WGS": "8", "PSSBAM_TILE_READS": "48"},
    "two_wg_overflow": {"PSSBAM_GRID_WGS": "2", "PSSBAM_TILE_READS": "64", "PSSBAM_PIECES": "5"},
    "simple_one_block": {"PSSBAM_SIMPLE_BLOCKS": "1"},
}


@pytest.fixture(scope="module")
def tiles(oracle, tmp_path_factory):
    case = Case(oracle, tmp_path_factory.mktemp("score_tiles"), *tl.fuzz_dataset(9601, 3200))
    assert_every_tile_overflows(tl.raw_records(case.refs, case.recs))      # with 5 pieces every tile of 64 holds an overflow record
    counts = np.array([len(b) for b in rs.split_by_bin(case.recs, case.contigs, TABLES["pmd"], 2, 8)])
    assert counts.min() >= 20 and counts[:1].sum() * 10 >= counts.sum() and counts[1:].sum() * 10 >= counts.sum()
    yield case
    case.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_several_tiles_per_workgroup(pkg, tiles, monkeypatch, shape):
    """filter S >= -256 with the four-bin histogram in one run: the LDS bins must survive the tile loop, and the records longer
    than the staging buffer take the one-lane path (read_score)"""
    for key, v in SHAPES[shape].items():
        monkeypatch.setenv(key, v)
    kernel = "SIMPLE" if shape == "simple_one_block" else "TILED"
    o = tl.PssOpts(region_len=15)
    tot, (sf, sr), _ = check_filter(pkg, tiles, o, kernel, "pmd", -256, half=2, shift=8)
    rows = tiles.ok_rows(o, "pmd", 2, 8)
    want = 2 * rows["unpaired"] + rows["first"] + rows["second"] + rows["other"]
    want[:1] = 0
    assert np.array_equal(sf + sr, want) and want[1:].all()
    assert all(sf[1:] >= (rows["unpaired"] + rows["first"])[1:]) and all(sr[1:] >= (rows["unpaired"] + rows["second"])[1:])
    if shape == "two_wg_overflow":
        assert tot.stats["slow_path"] >= 50


# ---- 7. feed and command ---------------------------------------------------------------------------------------------

def test_submit_bgzf(pkg, fuzz, tmp_path):
    """the compressed feed (device-indexed blocks) goes through the same launches; the setting follows feed_open"""
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, fuzz.refs, fuzz.recs, rng=np.random.default_rng(3))
    o = tl.PssOpts(region_len=15)
    wf, wr, wst = fuzz.reduced("pmd", -256, o)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(fuzz.refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_read_score(**setting("pmd", -256, 2, 8))
    eng.set_genome_arrays(tl.loaded_contigs(fuzz.contigs))
    eng.set_references([nm for nm, _ in fuzz.refs])
    sf, sr = eng.finish_read_score()
    tot = eng.finish()
    assert eng.feed_status()["flags"] == 0
    eng.close()
    assert np.array_equal(tot.fwd, wf) and np.array_equal(tot.rev, wr) and tot.stats["pss_ok"] == int(wst[tl.ST_OK])
    assert tot.stats["records"] == len(fuzz.recs)
    ref_tot, (rf, rr), _ = run_engine(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, pkg.KERNEL_TILED, setting("pmd", -256, 2, 8))
    assert np.array_equal(sf, rf) and np.array_equal(sr, rr) and sf[1:].all() and not sf[:1].any()
    same_but_slow_path(tot, ref_tot)


def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


def run_cli(pkg, fa, aln, prefix, *more, env=None):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), *more], capture_output=True, text=True,
                          env={**os.environ, **(env or {})}, timeout=300)


ROUTES = {"default": {}, "two_engines": {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"},
          "host_reader": {"PSSBAM_DEVICE_INFLATE": "0"}}


def host_weights(pkg) -> np.ndarray:
    """the table the command line passes to the engine"""
    host = C.CDLL(str(pkg.LIB_HOST))
    w = np.zeros((4, rs.PMD_DIST, rs.PMD_QUAL), dtype=np.int16)
    host.pss_pmd_weights.argtypes = [C.c_void_p]
    host.pss_pmd_weights.restype = None
    host.pss_pmd_weights(w.ctypes.data)
    return w


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("tag,base,t", [("pmd3_setD", "setD", "3"), ("pmd0_setA", "setA", "0")])
def test_cli_goldens(pkg, tmp_path, tag, base, t, route):
    """what the unmodified reference wrote for the reduced inputs (tests/golden/make_read_score_golden.py), byte for byte"""
    pr = run_cli(pkg, GOLD / f"{base}.fa", GOLD / f"{base}.bam", tmp_path / "out", "-y", t, env=ROUTES[route])
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(f" -y {t}")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.counts.txt", "out.pss.rates.txt"]
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"out.pss.{kind}.txt").read_text()) == report_body((GOLD / f"{tag}.pss.{kind}.txt").read_text()), kind


@pytest.mark.parametrize("route", list(ROUTES))
def test_cli_histogram_file(pkg, oracle, fuzz, tmp_path, route):
    """-Y (and -y -1 -Y) on the unpaired reads of the fuzz set, four copies: every row of the file is four times OK(bin) of the
    oracle on the records read_score_lib puts into that bin, in both columns; counts and rates are those without the option"""
    W = host_weights(pkg)
    TABLES["cli"] = W
    base = [r for r in tl.ref_safe(fuzz.recs) if not r.flag & 1]
    recs = [replace(r, qname=f"{r.qname}.{j}") for j in range(4) for r in base]
    fa, aln = tmp_path / "g.fa", tmp_path / "in.bam"
    tl.write_fasta(fa, fuzz.contigs)
    tl.write_bam(aln, fuzz.refs, recs, rng=np.random.default_rng(2))
    case = Case(oracle, tmp_path, fuzz.contigs, fuzz.refs, base)
    try:
        ok = case.ok_rows(tl.PssOpts(), "cli", rs.PMD_HALF, rs.PMD_SHIFT)["unpaired"]
    finally:
        case.close()
    assert (ok > 0).sum() >= 4 and ok[:32].any() and ok[32:].any()
    plain = run_cli(pkg, fa, aln, tmp_path / "plain", env=ROUTES[route])
    assert plain.returncode == 0, plain.stderr
    for args, first in ((["-Y"], 0), (["-y", "-1", "-Y"], 31)):
        pr = run_cli(pkg, fa, aln, tmp_path / "out", *args, env=ROUTES[route])
        assert pr.returncode == 0, pr.stderr
        assert pr.stderr.splitlines()[0].endswith(" " + " ".join(args))
        lines = (tmp_path / "out.pss.pmd.txt").read_text().splitlines()
        assert lines[0].startswith("# post-mortem-damage score") and lines[3] == "score\tfwd\trev" and len(lines) == 68
        rows = [ln.split("\t") for ln in lines[4:]]
        assert [r[0] for r in rows] == ["<-31"] + [str(v) for v in range(-31, 31)] + [">=31"]
        want = ok.copy()
        want[:first] = 0
        assert [int(r[1]) for r in rows] == [4 * int(v) for v in want] and [int(r[2]) for r in rows] == [4 * int(v) for v in want]
        if not first:
            for kind in ("counts", "rates"):
                assert report_body((tmp_path / f"out.pss.{kind}.txt").read_text()) == report_body((tmp_path / f"plain.pss.{kind}.txt").read_text())


def test_cli_sam_text_with_filters(pkg, oracle, tmp_path):
    """-y -0.5 together with -Q 20 -T <bed> -R <group> through SAM text input: the oracle (which has no -R of its own) on the
    group's records, reduced, masked and cut to the regions"""
    contigs, refs, recs = tl.fuzz_dataset(5, 1500, with_rg=True)
    recs = tl.ref_safe(recs)
    rg = "grpA"
    mine = [r for r in recs if ("RG", "Z", rg) in r.tags]
    assert 200 < len(mine) < len(recs) - 200
    ivs = rl.fuzz_intervals(5, contigs, recs)
    fa, aln, bed = tmp_path / "g.fa", tmp_path / "in.sam", tmp_path / "r.bed"
    tl.write_fasta(fa, contigs)
    tl.write_sam(aln, refs, recs)
    rl.write_bed(bed, ivs)
    W = host_weights(pkg)
    pr = run_cli(pkg, fa, aln, tmp_path / "out", "-y", "-0.5", "-Y", "-Q", "20", "-T", str(bed), "-R", rg)
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(" -Q 20 -y -0.5 -Y")
    kept = rl.reduce_recs(bq.mask_recs(rs.reduce_to(mine, contigs, W, -128, 20), 20), ivs)
    red = tmp_path / "red.sam"
    tl.write_sam(red, refs, kept)
    g = oracle.load_genome(fa)
    try:
        wf, wr, wst = oracle.pss(g, red, tl.PssOpts())
        tl.write_sam(red, refs, rl.reduce_recs(bq.mask_recs(mine, 20), ivs))
        pf, _, pst = oracle.pss(g, red, tl.PssOpts())
    finally:
        oracle.free_genome(g)
    gf, gr = tl.parse_counts_text((tmp_path / "out.pss.counts.txt").read_text())
    assert np.array_equal(gf, wf) and np.array_equal(gr, wr)
    assert 0 < int(wst[tl.ST_OK]) < int(pst[tl.ST_OK]) and wf[2:].sum() > 50
    rows = [ln.split("\t") for ln in (tmp_path / "out.pss.pmd.txt").read_text().splitlines()[4:]]
    assert not any(int(r[1]) or int(r[2]) for r in rows[:31]) and sum(int(r[1]) for r in rows) > 0           # nothing below -1 nat

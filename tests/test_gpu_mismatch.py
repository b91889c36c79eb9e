"""pss-bam -n / -N / -V on the GPU: the mismatch count of a whole read against the reference as a record filter and as
a histogram, counted in the tally kernels (tally_tiled's MISM arm; tally_simple and the tiled kernel's one-lane path
through count_mismatches).  The yardstick is the CPU oracle on reduced inputs built by mismatch_lib:

    filter k:     fwd, rev and PSS_OK == the oracle's on RED(k), the input without the <L>M records beyond k; every other
                  status slot and PSS_OK + PSS_FILTERED as the engine without the setting;
    histogram M:  with OK(b) the oracle's PSS_OK on the records whose min(m, M + 1) is b, per flag class as the length
                  histogram's tests have it -- unpaired mf[b] == mr[b] == OK(b), first mates mf only, second mates mr
                  only, any input mf[b] + mr[b] == 2 * OK_unpaired(b) + OK_paired(b); tables and stats untouched.

Bit-exact (integer work).  test_mismatch_host.py asserts without a GPU that no comparison here is vacuous."""
import os
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import mismatch_lib as ml
import pssbam_testlib as tl
import regions_lib as rl
from test_gpu_length_hist import CLASSES, pss_dict, same_but_slow_path, split_by_flag
from test_gpu_tile_loop import assert_every_tile_overflows

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
KERNELS = ["SIMPLE", "TILED"]
OTHER_SLOTS = ("records", "rg_dropped", "parse_skip", "no_contig")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def kern(pkg, name):
    return {"SIMPLE": pkg.KERNEL_SIMPLE, "TILED": pkg.KERNEL_TILED, "AUTO": pkg.KERNEL_AUTO}[name]


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, mism=None, regions=None, **kw):
    """-> (totals, (mf, mr) or None, n_u64)"""
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, mismatches=mism, **kw)
    assert eng.mismatches == (None if mism is None or (mism[0] == 0 and mism[1] < 0) else (mism[0], mism[1], int(bool(mism[2]))))
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if regions is not None:
        eng.set_regions(*rl.to_arrays(regions))
    if recs:
        eng.submit(tl.raw_records(refs, recs))
    hist = eng.finish_mismatches() if mism is not None and mism[0] else None
    tot = eng.finish()
    n_u64 = eng.counters_device()[1]
    eng.close()
    if hist is not None:
        assert hist[0].shape == hist[1].shape == (mism[0] + 2,) and hist[0].dtype == np.uint64
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

    def reduced(self, k: int, tv: bool, o: tl.PssOpts, q: int = 0, ivs=None):
        """the oracle on RED(k) -- masked at base quality q and reduced to the regions, where given"""
        key = (k, tv, o.region_len, q, ivs is not None)
        if key not in self._orc:
            recs = ml.reduce_to(self.recs, self.ctg, k, tv)      # m is taken from SEQ as stored: reduce first, mask then
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

    def ok_rows(self, o: tl.PssOpts, M: int, tv: bool) -> dict:
        """{flag class: OK(b) for b = 0 .. M + 1} from the oracle on every (class, bin) subset that holds a record"""
        key = (o.region_len, M, tv)
        if key not in self._rows:
            rows = {}
            for c, part in split_by_flag(self.recs).items():
                rows[c] = np.zeros(M + 2, dtype=np.uint64)
                for b, sub in enumerate(ml.split_by_bin(part, self.ctg, M, tv)):
                    if sub:
                        rows[c][b] = self.oracle_on(sub, o)[2][tl.ST_OK]
            self._rows[key] = rows
        return self._rows[key]


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    case = Case(oracle, tmp_path_factory.mktemp("mism"), *tl.fuzz_dataset(7301, 3000))
    yield case
    case.close()


def check_filter(pkg, case: Case, o, kernel: str, k: int, tv: bool, q: int = 0, ivs=None, hist_max: int = 0):
    """one engine run with the filter against the oracle on RED(k) and the engine without the setting"""
    wf, wr, wst = case.reduced(k, tv, o, q, ivs)
    plain = case.plain(pkg, o, kernel, q, ivs)
    tot, hist, _ = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), (hist_max, k, tv), ivs, min_base_qual=q)
    assert np.array_equal(tot.fwd, wf) and np.array_equal(tot.rev, wr), (k, tv, o.region_len, kernel)
    assert tot.stats["pss_ok"] == int(wst[tl.ST_OK])
    for slot in OTHER_SLOTS:
        assert tot.stats[slot] == plain.stats[slot], slot
    assert tot.stats["pss_ok"] + tot.stats["pss_filtered"] == plain.stats["pss_ok"] + plain.stats["pss_filtered"]
    return tot, hist, plain


# ---- 1. filter parity ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [0, 15, 30])
@pytest.mark.parametrize("tv", [False, True], ids=["all", "tv"])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_filter_parity(pkg, fuzz, k, tv, n, kernel):
    tot, _, plain = check_filter(pkg, fuzz, tl.PssOpts(region_len=n), kernel, k, tv)
    assert 0 < tot.stats["pss_ok"] < plain.stats["pss_ok"]              # the filter bites and leaves something


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_with_min_base_quality(pkg, fuzz, kernel):
    """-Q masks table positions and does not change m: the oracle runs on RED(k) masked afterwards"""
    o = tl.PssOpts(region_len=15)
    tot, _, plain = check_filter(pkg, fuzz, o, kernel, 1, False, q=20)
    assert not np.array_equal(plain.fwd, fuzz.plain(pkg, o, kernel).fwd)    # the mask did bite
    unmasked = fuzz.reduced(1, False, o)
    assert tot.stats["pss_ok"] == int(unmasked[2][tl.ST_OK]) and not np.array_equal(tot.fwd, unmasked[0])


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_with_regions(pkg, fuzz, kernel):
    ivs = rl.fuzz_intervals(7301, fuzz.contigs, fuzz.recs)
    o = tl.PssOpts(region_len=15)
    tot, _, plain = check_filter(pkg, fuzz, o, kernel, 1, True, ivs=ivs)
    assert 0 < tot.stats["pss_ok"] < plain.stats["pss_ok"] < fuzz.plain(pkg, o, kernel).stats["pss_ok"]


# ---- 2. histogram identities -----------------------------------------------------------------------------------------

def check_identities(pkg, case: Case, o, kernel: str, M: int, k: int = -1, tv: bool = False):
    """the per-class identities on the engine run over each subset, the sum identity on the run over all records, and
    tables + stats against an engine with the same filter and no histogram; rows above k must be zero"""
    want = {c: v.copy() for c, v in case.ok_rows(o, M, tv).items()}
    if k >= 0:
        for v in want.values():
            v[k + 1:] = 0
    zero = np.zeros(M + 2, dtype=np.uint64)
    parts = split_by_flag(case.recs)
    for c in CLASSES:
        _, (mf, mr), _ = run_engine(pkg, case.contigs, case.refs, parts[c], o, kern(pkg, kernel), (M, k, tv))
        if c == "unpaired":
            assert np.array_equal(mf, want[c]) and np.array_equal(mr, want[c]), (c, M, k)
        elif c == "first":
            assert np.array_equal(mf, want[c]) and np.array_equal(mr, zero), (c, M, k)
        elif c == "second":
            assert np.array_equal(mr, want[c]) and np.array_equal(mf, zero), (c, M, k)
        else:
            assert np.array_equal(mf + mr, want[c]), (c, M, k)
    tot, (mf, mr), n_u64 = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), (M, k, tv))
    paired = want["first"] + want["second"] + want["other"]
    assert np.array_equal(mf + mr, 2 * want["unpaired"] + paired)
    assert np.array_equal(mf >= want["unpaired"] + want["first"], np.ones(M + 2, dtype=bool))
    assert np.array_equal(mr >= want["unpaired"] + want["second"], np.ones(M + 2, dtype=bool))
    if k >= 0:
        assert not mf[k + 1:].any() and not mr[k + 1:].any()
        same, _, n_plain = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), (0, k, tv))
    else:
        same, n_plain = case.plain(pkg, o, kernel), None
    same_but_slow_path(tot, same)
    assert int(mf.sum()) + int(mr.sum()) == 2 * tot.stats["pss_ok"] - int(paired.sum())   # an unpaired read counts in both arrays
    if n_plain is not None:
        assert n_u64 == n_plain + 2 * (M + 2)
    return mf, mr, tot


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("k", [-1, 1], ids=["no_filter", "k1"])
@pytest.mark.parametrize("M", [4, 255])
def test_histogram_identities(pkg, fuzz, M, k, kernel):
    mf, mr, _ = check_identities(pkg, fuzz, tl.PssOpts(region_len=15), kernel, M, k)
    top = M + 2 if k < 0 else k + 1
    assert all(mf[:min(top, 4)] > 0) and all(mr[:min(top, 4)] > 0) and not np.array_equal(mf, mr)
    if k < 0 and M == 4:
        assert mf[5] > 0 and mr[5] > 0                                   # the ">M" row


def test_histogram_transversions_only(pkg, fuzz):
    mf, _, _ = check_identities(pkg, fuzz, tl.PssOpts(region_len=15), "TILED", 4, -1, True)
    af, _, _ = check_identities(pkg, fuzz, tl.PssOpts(region_len=15), "TILED", 4)
    assert mf[0] > af[0] and mf.sum() == af.sum()


# ---- 3. off is off ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS + ["AUTO"])
def test_off_is_off(pkg, fuzz, kernel):
    o = tl.PssOpts(region_len=15)
    plain = fuzz.plain(pkg, o, kernel)
    eng = pkg.Engine(pss=pss_dict(o), kernel=kern(pkg, kernel))
    n_plain = eng.counters_device()[1]
    eng.set_mismatches(4, 1, 1)
    assert eng.counters_device()[1] == n_plain + 12 == eng.counter_layout()["n_u64"]
    assert eng.counter_layout()["mism_fwd"] == n_plain and eng.counter_layout()["mism_rev"] == n_plain + 6
    eng.set_mismatches(0, -1, 0)
    assert eng.mismatches is None and eng.counters_device()[1] == n_plain == eng.counter_layout()["n_u64"]
    with pytest.raises(pkg.PssbamError):
        eng.finish_mismatches()
    eng.set_genome_arrays(tl.loaded_contigs(fuzz.contigs))
    eng.set_references([nm for nm, _ in fuzz.refs])
    eng.submit(tl.raw_records(fuzz.refs, fuzz.recs))
    tot = eng.finish()
    eng.close()
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev) and tot.stats == plain.stats
    # k = 255: no read of the set is that far from the reference
    far, _, n_far = run_engine(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, kern(pkg, kernel), (0, 255, 0))
    assert n_far == n_plain
    same_but_slow_path(far, plain)


def test_rules(pkg):
    E = pkg.PssbamError
    for bad in ((256, -1, 0), (-1, -1, 0), (0, 256, 0), (0, -2, 0), (4, 1 << 20, 1)):
        with pytest.raises(E):
            pkg.Engine(pss=dict(region_len=5), mismatches=bad)
    with pytest.raises(E):                                  # nothing is added to a table on a k-mer engine
        pkg.Engine(kmer=dict(klen=4), mismatches=(4, 1, 0))
    with pytest.raises(E):
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), mismatches=(0, 1, 0))
    with pytest.raises(E):                                  # the decision is taken in the one pass that holds all rows
        pkg.Engine(pss=dict(region_len=31), mismatches=(0, 1, 0))
    others = (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]}), dict(length_hist=100),
              dict(site_context="cpg"), dict(end_condition=(1, 13, 13)), dict(gapped=True), dict(per_contig=True))
    for kw in others:
        eng = pkg.Engine(pss=dict(region_len=5), **kw)
        for mism in ((4, -1, 0), (0, 1, 0)):
            with pytest.raises(E):
                eng.set_mismatches(*mism)
        assert eng.mismatches is None
        eng.set_mismatches(0, -1, 0)                        # switching off what is off is always legal
        eng.close()
    for mism in ((4, -1, 0), (0, 1, 1)):
        eng = pkg.Engine(pss=dict(region_len=5), mismatches=mism)
        for setter, args in ((eng.set_read_groups, (["a"],)), (eng.set_length_bins, ([30],)), (eng.set_contig_sets, ({"x": ["chrA"]},)),
                             (eng.set_length_histogram, (100,)), (eng.set_site_context, ("cpg",)), (eng.set_end_condition, (1, 13, 13)),
                             (eng.set_gapped, (True,)), (eng.set_per_contig, (True,))):
            with pytest.raises(E):
                setter(*args)
        assert eng.mismatches == mism
        eng.set_mismatches(0, -1, 0)
        eng.set_length_histogram(100)                       # off again: the others are legal
        eng.close()

    eng = pkg.Engine(pss=dict(region_len=5), read_group="grpA", min_base_qual=10, mismatches=(10, 3, 1))   # goes with -R and -Q
    lay = eng.counter_layout()
    assert lay["mism_fwd"] == lay["stats"] + pkg.ST_N and lay["mism_rev"] == lay["mism_fwd"] + 12
    assert lay["n_u64"] == lay["mism_rev"] + 12 == eng.counters_device()[1]
    contigs, refs, recs = tl.fuzz_dataset(5, 300, with_rg=True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    for mism in ((0, -1, 0), (10, 3, 1), (4, 1, 0)):
        with pytest.raises(E):                              # records have been tallied
            eng.set_mismatches(*mism)
    first = eng.finish_mismatches()
    assert first[0].sum() > 0
    eng.reset()                                             # the setting survives reset
    assert eng.counters_device()[1] == lay["n_u64"]
    zf, zr = eng.finish_mismatches()
    assert not zf.any() and not zr.any()
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_mismatches()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    eng.reset()
    eng.set_mismatches(4, -1, 0)                            # legal again after reset
    assert eng.counters_device()[1] == eng.counter_layout()["n_u64"] == lay["mism_fwd"] + 12
    eng.close()

    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_mismatches(4, -1, 0)
    eng.set_mismatches(0, 2, 0)                             # the filter alone adds no words
    assert eng.counters_device() == (d, n)
    eng.close()
    other.close()


# ---- 4. edges ----------------------------------------------------------------------------------------------------------

EDGE_LENGTHS = (7, 8, 9, 16, 17, 31, 32, 33, 150)


def lane_cut(n: int) -> int:
    """where the tiled kernel cuts a read of n compared bases between the two lanes of its pair"""
    return min(n, ((n >> 1) + 7) & ~7)


def edge_contigs():
    clean = ml.clean_contig(6000, seed=21)
    odd = list(ml.clean_contig(3000, seed=22))
    odd[1000:1100] = "".join(odd[1000:1100]).lower()                     # lower case: folded, counts like upper case
    for p in range(1200, 1245, 7):                                       # (the reads over them end at 1250 .. 1257: clean context bases)
        odd[p] = "N"
    for p in range(1203, 1245, 7):
        odd[p] = "Y"
    return [("c", clean), ("odd", "".join(odd))]


def edge_groups():
    """{name: (region_len, [records])}: every record is added to both tables (or, paired, to one) without the filter"""
    (_, clean), (_, odd) = edge_contigs()
    G, n = {}, [0]

    def name():                                                            # read names of every length mod 4: the record's offset in the block
        n[0] += 1
        return f"e{n[0]:04d}" + "x" * (n[0] % 4)

    pos = []
    for L in EDGE_LENGTHS:
        cut = lane_cut(L)
        for a in range(8):                                                 # contig start s with s mod 8 = 0..7
            s = 40 + 16 * L + a
            spots = sorted({0, L - 1, max(cut - 1, 0), min(cut, L - 1), 7 if L > 7 else 0, 8 if L > 8 else 0})
            pos += [ml.with_mismatches(clean, s, L, [p], name=name()) for p in spots]
            pos.append(ml.with_mismatches(clean, s, L, range(L), name=name()))          # m = L: a bin of its own per length
            pos.append(ml.with_mismatches(clean, s, L, range(0, L, 3), name=name()))
            pos.append(ml.read_on(clean, s, L, name=name()))
    G["positions"] = (5, pos)
    G["length_one"] = (0, [ml.with_mismatches(clean, 500 + a, 1, p, name=name()) for a in range(8) for p in ([], [0])])
    G["boundary"] = (5, [ml.with_mismatches(clean, 900 + 37 * j + m, 40, range(0, 4 * m, 4), name=name()) for j in range(6) for m in (0, 1, 3, 4)])
    subs = []
    for ref_b in "ACGT":
        for read_b in "ACGT":
            if read_b != ref_b:
                s = next(p for p in range(2000 + 40 * len(subs), 5000) if clean[p + 20] == ref_b)
                subs.append(ml.read_on(clean, s, 40, {20: read_b}, name=name()))
    assert len(subs) == 12
    G["substitutions"] = (5, subs)
    quiet = []
    for a in range(8):
        s = 100 + 50 * a + a
        quiet.append(ml.read_on(clean, s, 40, {3: "N", 11: "R", 20: "=", 39: "N"}, name=name()))                  # in the read
        quiet.append(ml.read_on(clean, s, 40, {3: "N", 11: "R", 20: "=", 30: ml.OTHER[clean[s + 30]]}, name=name()))
        quiet.append(ml.read_on(odd, 1190 + a, 60, name=name(), rname="odd"))                                       # N and Y in the reference
        quiet.append(ml.read_on(odd, 1190 + a, 60, {i: "A" for i in range(60)}, name=name(), rname="odd"))
        quiet.append(ml.read_on(odd, 1010 + a, 50, name=name(), rname="odd"))                                       # lower case in the reference
        quiet.append(ml.with_mismatches(odd, 1010 + a, 50, [0, 17, 49], name=name(), rname="odd"))
    G["non_counting"] = (5, quiet)
    flags = []
    for a in range(8):
        s, L = 3000 + 60 * a + a, 44
        for fl, tlen in ((16, 0), (0x1 | 0x2 | 0x40, L), (0x1 | 0x2 | 0x80, -L), (0x1 | 0x2 | 0x40 | 0x10, -L), (0x1 | 0x2 | 0x80 | 0x10, L)):
            flags += [ml.with_mismatches(clean, s, L, [1, 30], name=name(), flag=fl, tlen=tlen), ml.read_on(clean, s, L, name=name(), flag=fl, tlen=tlen)]
    G["flags"] = (5, flags)
    G["beyond_255"] = (5, [ml.with_mismatches(clean, 4000 + a, 300, range(300), name=name()) for a in range(8)] +
                          [ml.with_mismatches(clean, 4000 + a, 300, range(255), name=name()) for a in range(2)] +
                          [ml.with_mismatches(clean, 4000 + a, 300, range(256), name=name()) for a in range(2)])
    # l_seq shorter than L: a first mate whose |TLEN| and CIGAR say 50 and whose SEQ holds 33, 40 or 41 bases
    G["short_seq"] = (5, [ml.with_mismatches(clean, 5000 + 11 * a, 50, spots, name=name(), flag=0x1 | 0x2 | 0x40, tlen=50, seq_len=n_seq)
                          for a in range(8) for n_seq in (33, 40, 41) for spots in ([], [0, n_seq - 1], [5])])
    return G


@pytest.fixture(scope="module")
def edges(oracle, tmp_path_factory):
    contigs = edge_contigs()
    refs = [(nm, len(s)) for nm, s in contigs]
    cases = {nm: (n, Case(oracle, tmp_path_factory.mktemp(f"edge_{nm}"), contigs, refs, recs)) for nm, (n, recs) in edge_groups().items()}
    yield cases
    for _, c in cases.values():
        c.close()


def edge_expectation(case: Case, M: int, tv: bool):
    """(mf, mr) straight from mismatch_lib: every record of an edge group is added to both tables, a mate to its own"""
    mf, mr = np.zeros(M + 2, dtype=np.uint64), np.zeros(M + 2, dtype=np.uint64)
    for r in case.recs:
        b = min(ml.mismatches(r, case.ctg, tv), M + 1)
        mf[b] += 0 if (r.flag & 0x81) == 0x81 else 1
        mr[b] += 0 if (r.flag & 0x41) == 0x41 else 1
    return mf, mr


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("tv", [False, True], ids=["all", "tv"])
@pytest.mark.parametrize("group", ["positions", "length_one", "boundary", "substitutions", "non_counting", "flags", "beyond_255", "short_seq"])
def test_edges(pkg, edges, group, tv, kernel):
    n, case = edges[group]
    o = tl.PssOpts(region_len=n)
    want_f, want_r = edge_expectation(case, 255, tv)
    tot, (mf, mr), _ = run_engine(pkg, case.contigs, case.refs, case.recs, o, kern(pkg, kernel), (255, -1, tv))
    assert np.array_equal(mf, want_f) and np.array_equal(mr, want_r), (np.flatnonzero(mf != want_f), np.flatnonzero(mr != want_r))
    assert tot.stats["pss_ok"] == len(case.recs) and tot.stats["pss_filtered"] == 0       # nothing else filters them
    rows = case.ok_rows(o, 255, tv)                                                          # and the oracle agrees, class by class
    assert np.array_equal(mf + mr, 2 * rows["unpaired"] + rows["first"] + rows["second"] + rows["other"])
    same_but_slow_path(tot, case.plain(pkg, o, kernel))
    for k in {"boundary": (0, 3), "beyond_255": (255, 254), "substitutions": (0,)}.get(group, (0,)):
        ftot, fh, _ = check_filter(pkg, case, o, kernel, k, tv, hist_max=255)
        kept = sum(1 for r in case.recs if ml.mismatches(r, case.ctg, tv) <= k)
        assert ftot.stats["pss_ok"] == kept and ftot.stats["pss_filtered"] == len(case.recs) - kept
        wf, wr = want_f.copy(), want_r.copy()
        wf[k + 1:] = 0
        wr[k + 1:] = 0
        assert np.array_equal(fh[0], wf) and np.array_equal(fh[1], wr)


def test_edge_groups_hold_what_they_claim():
    """(no GPU work) the hand-built records against the definition: the expected bins are the intended ones"""
    G = edge_groups()
    ctg = dict(edge_contigs())
    m = lambda r, tv=False: ml.mismatches(r, ctg, tv)     # noqa: E731
    assert all(m(r) is not None for _, recs in G.values() for r in recs)
    assert {len(r.qname) % 4 for r in G["positions"][1]} == {0, 1, 2, 3} and {(r.pos - 1) % 8 for r in G["positions"][1]} == set(range(8))
    assert {m(r) for r in G["positions"][1]} >= {0, 1, *EDGE_LENGTHS}
    assert sorted({m(r) for r in G["length_one"][1]}) == [0, 1] and sorted({m(r) for r in G["boundary"][1]}) == [0, 1, 3, 4]
    assert [m(r) for r in G["substitutions"][1]] == [1] * 12 and sum(m(r, True) for r in G["substitutions"][1]) == 8
    assert {m(r) for r in G["beyond_255"][1]} == {300, 255, 256}
    assert all(len(r.seq) < 50 == abs(r.tlen) for r in G["short_seq"][1]) and {m(r) for r in G["short_seq"][1]} == {0, 1, 2}
    quiet = G["non_counting"][1]
    assert [m(r) for r in quiet[:6]] == [0, 1, 0, m(quiet[3]), 0, 3] and 20 < m(quiet[3]) < 60     # N / Y columns never count


# ---- 5. several tiles per workgroup and the one-lane path -------------------------------------------------------------

SHAPES = {
    "one_wg": {"PSSBAM_GRID_WGS": "1", "PSSBAM_TILE_READS": "48"},
    "three_wg": {"PSSBAM_GRID_WGS": "3", "PSSBAM_TILE_READS": "48"},
    "xcd8": {"PSSBAM_XCD_MAP": "1", "PSSBAM_GRID_WGS": "8", "PSSBAM_TILE_READS": "48"},
    "two_wg_overflow": {"PSSBAM_GRID_WGS": "2", "PSSBAM_TILE_READS": "64", "PSSBAM_PIECES": "5"},
    "simple_one_block": {"PSSBAM_SIMPLE_BLOCKS": "1"},
}


@pytest.fixture(scope="module")
def tiles(oracle, tmp_path_factory):
    case = Case(oracle, tmp_path_factory.mktemp("mism_tiles"), *tl.fuzz_dataset(9601, 3200))
    assert_every_tile_overflows(tl.raw_records(case.refs, case.recs))      # with 5 pieces every tile of 64 holds an overflow record
    counts = ml.bin_counts(case.recs, case.contigs, 4)
    assert counts.min() >= 20 and counts[:2].sum() * 10 >= counts.sum() and counts[2:].sum() * 10 >= counts.sum()
    yield case
    case.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_several_tiles_per_workgroup(pkg, tiles, monkeypatch, shape):
    """filter k = 1 with histogram M = 4 in one run: the LDS bins must survive the tile loop"""
    for key, v in SHAPES[shape].items():
        monkeypatch.setenv(key, v)
    kernel = "SIMPLE" if shape == "simple_one_block" else "TILED"
    o = tl.PssOpts(region_len=15)
    tot, (mf, mr), _ = check_filter(pkg, tiles, o, kernel, 1, False, hist_max=4)
    rows = tiles.ok_rows(o, 4, False)
    want = 2 * rows["unpaired"] + rows["first"] + rows["second"] + rows["other"]
    want[2:] = 0
    assert np.array_equal(mf + mr, want) and want[:2].all()
    assert all(mf[:2] >= (rows["unpaired"] + rows["first"])[:2]) and all(mr[:2] >= (rows["unpaired"] + rows["second"])[:2])
    if shape == "two_wg_overflow":
        assert tot.stats["slow_path"] >= 50


# ---- 6. feed and command ---------------------------------------------------------------------------------------------

def test_submit_bgzf(pkg, fuzz, tmp_path):
    """the compressed feed (device-indexed blocks) goes through the same launches; the setting follows feed_open"""
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, fuzz.refs, fuzz.recs, rng=np.random.default_rng(3))
    o = tl.PssOpts(region_len=15)
    wf, wr, wst = fuzz.reduced(1, False, o)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(fuzz.refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_mismatches(4, 1, 0)
    eng.set_genome_arrays(tl.loaded_contigs(fuzz.contigs))
    eng.set_references([nm for nm, _ in fuzz.refs])
    mf, mr = eng.finish_mismatches()
    tot = eng.finish()
    assert eng.feed_status()["flags"] == 0
    eng.close()
    assert np.array_equal(tot.fwd, wf) and np.array_equal(tot.rev, wr) and tot.stats["pss_ok"] == int(wst[tl.ST_OK])
    assert tot.stats["records"] == len(fuzz.recs)
    ref_tot, (rf, rr), _ = run_engine(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, pkg.KERNEL_TILED, (4, 1, 0))
    assert np.array_equal(mf, rf) and np.array_equal(mr, rr) and mf[:2].all() and not mf[2:].any()
    same_but_slow_path(tot, ref_tot)


def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


def run_cli(pkg, fa, aln, prefix, *more, env=None):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), *more], capture_output=True, text=True,
                          env={**os.environ, **(env or {})}, timeout=300)


@pytest.mark.parametrize("tag,base,args", [("mism1_setA", "setA", ["-n", "1"]), ("mismtv0_setD", "setD", ["-n", "0", "-V"])])
def test_cli_goldens(pkg, tmp_path, tag, base, args):
    """what the unmodified reference wrote for the reduced inputs (tests/golden/make_mismatch_golden.py), byte for byte"""
    pr = run_cli(pkg, GOLD / f"{base}.fa", GOLD / f"{base}.bam", tmp_path / "out", *args)
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(" " + " ".join(args))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.counts.txt", "out.pss.rates.txt"]
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"out.pss.{kind}.txt").read_text()) == report_body((GOLD / f"{tag}.pss.{kind}.txt").read_text()), kind


def setA():
    import site_context_lib as sc
    contigs = sc.read_fasta(GOLD / "setA.fa")
    refs, recs = ml.read_sam(GOLD / "setA.sam")
    return contigs, refs, recs


def expected_file(pkg, oracle, tmp_path, contigs, refs, recs, fa, aln, M, k, tv) -> bytes:
    """the mismatches file pss_write_mismatches writes from mismatch_lib's bins and the oracle's OK counts"""
    import ctypes as C
    case = Case(oracle, tmp_path, contigs, refs, recs)
    try:
        rows = case.ok_rows(tl.PssOpts(), M, tv)
    finally:
        case.close()
    mf, mr = rows["unpaired"] + rows["first"], rows["unpaired"] + rows["second"]
    # a record with both or neither of 0x40 / 0x80 goes to one table, which OK alone does not tell: one oracle run each
    case = Case(oracle, tmp_path, contigs, refs, recs)
    try:
        for b, sub in enumerate(ml.split_by_bin(split_by_flag(recs)["other"], case.ctg, M, tv)):
            for r in sub if rows["other"][b] else []:
                f1, r1, st = case.oracle_on([r], tl.PssOpts())
                assert int(st[tl.ST_OK]) == int(f1.any()) + int(r1.any()) <= 1
                mf[b] += int(f1.any())
                mr[b] += int(r1.any())
    finally:
        case.close()
    assert int(mf.sum() + mr.sum()) == int(sum(2 * rows["unpaired"] + rows["first"] + rows["second"] + rows["other"]))
    if k >= 0:
        mf[k + 1:] = 0
        mr[k + 1:] = 0
    host = C.CDLL(str(pkg.LIB_HOST))
    host.pss_write_mismatches.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert host.pss_write_mismatches(str(fa).encode(), str(aln).encode(), str(tmp_path / "want").encode(), M, int(tv), mf.ctypes.data, mr.ctypes.data) == 0
    assert mf[:2].all() and mr[:2].all()
    return (tmp_path / "want.pss.mismatches.txt").read_bytes()


def test_cli_histogram(pkg, oracle, tmp_path):
    """-N 4 on setA.bam: the mismatches file, and counts / rates unchanged (pss_0 of the same options)"""
    fa, aln = GOLD / "setA.fa", GOLD / "setA.bam"
    pr = run_cli(pkg, fa, aln, tmp_path / "out", "-N", "4")
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(" -N 4")
    assert sorted(p.name for p in tmp_path.glob("out.*")) == ["out.pss.counts.txt", "out.pss.mismatches.txt", "out.pss.rates.txt"]
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"out.pss.{kind}.txt").read_text()) == report_body((GOLD / f"pss_0.pss.{kind}.txt").read_text()), kind
    contigs, refs, recs = setA()
    want = expected_file(pkg, oracle, tmp_path, contigs, refs, recs, fa, aln, 4, -1, False)
    assert (tmp_path / "out.pss.mismatches.txt").read_bytes() == want
    assert want.startswith(b"# mismatches (all) of the reads added to the forward / reverse table\n")


def test_cli_sam_text_with_everything(pkg, oracle, tmp_path):
    """-N 4 -n 1 -V through SAM text input"""
    fa, aln = GOLD / "setA.fa", GOLD / "setA.sam"
    pr = run_cli(pkg, fa, aln, tmp_path / "out", "-N", "4", "-n", "1", "-V")
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(" -n 1 -N 4 -V")
    contigs, refs, recs = setA()
    want = expected_file(pkg, oracle, tmp_path, contigs, refs, recs, fa, aln, 4, 1, True)
    assert (tmp_path / "out.pss.mismatches.txt").read_bytes() == want
    assert want.startswith(b"# mismatches (transversions only) of the reads")
    reduced = tmp_path / "red.sam"
    reduced.write_text(ml.reduce_sam_text(aln.read_text(), contigs, 1, True))
    g = oracle.load_genome(fa)
    try:
        wf, wr, _ = oracle.pss(g, reduced, tl.PssOpts())
    finally:
        oracle.free_genome(g)
    gf, gr = tl.parse_counts_text((tmp_path / "out.pss.counts.txt").read_text())
    assert np.array_equal(gf, wf) and np.array_equal(gr, wr) and wf[2:].sum() > 100


@pytest.mark.parametrize("env", [{"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}, {"PSSBAM_DEVICE_INFLATE": "0"}],
                         ids=["two_engines", "host_reader"])
def test_cli_other_routes(pkg, fuzz, tmp_path, env):
    """two engines whose counter blocks are summed, and the host reader: the three files of the default route, byte for byte"""
    recs = [replace(r, qname=f"{r.qname}.{j}") for j in range(4) for r in tl.ref_safe(fuzz.recs)]     # a few batches of 1 MiB
    fa, aln = tmp_path / "g.fa", tmp_path / "in.bam"
    tl.write_fasta(fa, fuzz.contigs)
    tl.write_bam(aln, fuzz.refs, recs, rng=np.random.default_rng(2))
    outs = {}
    for tag, e in (("one", {}), ("other", env)):
        pr = run_cli(pkg, fa, aln, tmp_path / "out", "-N", "4", "-n", "3", env=e)
        assert pr.returncode == 0, pr.stderr
        outs[tag] = {kind: (tmp_path / f"out.pss.{kind}.txt").read_bytes() for kind in ("counts", "rates", "mismatches")}
    assert outs["one"] == outs["other"]
    rows = [ln.split("\t") for ln in outs["one"]["mismatches"].decode().splitlines()[4:]]
    assert [r[0] for r in rows] == ["0", "1", "2", "3", "4", ">4"] and all(int(r[1]) > 0 and int(r[2]) > 0 for r in rows[:4])
    assert [r[1:] for r in rows[4:]] == [["0", "0"], ["0", "0"]]
    _, (mf, mr), _ = run_engine(pkg, fuzz.contigs, fuzz.refs, tl.ref_safe(fuzz.recs), tl.PssOpts(), pkg.KERNEL_TILED, (4, 3, 0))
    assert [int(r[1]) for r in rows] == [4 * int(v) for v in mf] and [int(r[2]) for r in rows] == [4 * int(v) for v in mr]

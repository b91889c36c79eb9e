"""Depth of coverage of the kept records (pssbam_engine_set_coverage) on the GPU, through the Engine wrapper.  The expected side
of every test is coverage_lib, the Python restatement, over the records that the record sink of the SAME run delivers: per-contig
figures, the histogram and the runs must be exactly equal."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import __graft_entry__ as ge
import coverage_lib as cl
import duplicates_lib as dl
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = "pssbam error -1:", "pssbam error -5:"
TILE, SUMS_ROUND = 4096, 256      # csrc/coverage_kernels.h: COV_TILE, COV_SUMS_ROUND
PAD = 256                         # csrc/engine.hip: the first contig starts CONTIG_PAD positions into the genome's index space
# the figures of the commit before the setting existed, for OFF_INPUT with the setting off: pssbam_engine_kernel_time's launch count
# and the counter block's words
OFF_INPUT = (7, 3000)             # tl.fuzz_dataset(seed, n_reads), one submit, pss region_len 15
OFF_LAUNCHES, OFF_N_U64 = 1, 560


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    assert hasattr(p.hip_lib(), "pssbam_engine_set_coverage")
    return p


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq, up_ctx=o.up_ctx,
                down_ctx=o.down_ctx, merged_only=o.merged_only)


def acgt(rng, n) -> str:
    """upper-case A C G T only: every candidate read on it passes the default -U / -D contexts"""
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, size=n)])


class Case:
    def __init__(self, contigs, refs, recs, pss, **setup):
        self.contigs, self.refs, self.recs = contigs, refs, recs
        self.lens = {n: len(s) for n, s in contigs}
        self.setup = dl.Setup(refs, self.lens, pss=pss, **setup)
        self.raw = tl.raw_records(refs, recs)
        self._loaded = None

    def loaded(self):
        if self._loaded is None:
            self._loaded = tl.loaded_contigs(self.contigs)
        return self._loaded

    def engine(self, pkg, **kw):
        return pkg.Engine(pss=pss_dict(self.setup.pss), read_group=self.setup.read_group, **kw)

    def genome(self, eng):
        eng.set_genome_arrays(self.loaded())
        eng.set_references([n for n, _ in self.refs])

    def model_kept(self):
        idx = {n: i for i, (n, _) in enumerate(self.refs)}
        return np.array([cl.kept(cl.core_of_rec(r, idx), self.setup) for r in self.recs])


def blocks_of(pkg, raw, cuts):
    offs = pkg.index_records(raw)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            o = offs[a:b + 1].astype(np.int64)
            out.append((raw[o[0]:o[-1]], (o - o[0]).astype(np.uint32)))
    return out


def collect(eng, c: Case):
    """-> (per_contig, hist, n_runs, runs, kept) of everything since create / reset; kept = the sink's records since the last call"""
    per, hist, n_runs = eng.finish_coverage(len(c.refs))
    runs = eng.finish_coverage_runs()
    return per, hist, n_runs, runs, eng.finish_records()


def check(c: Case, got, kept_raw=None):
    per, hist, n_runs, runs, kept = got
    want = cl.from_raw(kept if kept_raw is None else kept_raw, c.refs, c.lens)
    assert np.array_equal(per, want.per_contig), (per, want.per_contig)
    assert np.array_equal(hist, want.hist)
    assert n_runs == want.n_runs == len(runs[0])
    for x, y in zip(runs, want.runs):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    return want


def run(pkg, c: Case, raw=None, cuts=None, before=None, **kw):
    raw = c.raw if raw is None else raw
    eng = c.engine(pkg, **kw)
    try:
        if before:
            before(eng)
        eng.set_coverage(True, sum(ln for _, ln in c.refs))
        eng.set_record_sink()
        c.genome(eng)
        eng.kernel_time()
        n = pkg.index_records(raw).size - 1
        for blk, offs in blocks_of(pkg, raw, cuts or [0, n]):
            eng.submit(blk, offs)
        return collect(eng, c)
    finally:
        eng.close()


# ---- the data ------------------------------------------------------------------------------------------------------------------------

def read(c_seq, name, rname, pos0, L, **kw):
    return tl.Rec(**{**dict(qname=name, flag=0, rname=rname, pos=pos0 + 1, mapq=40, cigar=[(L, "M")], seq=c_seq[pos0:pos0 + L], qual="I" * L), **kw})


_CASES: dict = {}


def small_case() -> Case:
    """contigs of 1, 255, 256, 257 and 5000 bases -- several share one scan tile -- listed in the header against the genome's (name)
    order and beside a reference the genome lacks; reads in every category"""
    if "small" not in _CASES:
        rng = np.random.default_rng(71)
        contigs = [("e1", acgt(rng, 1)), ("d255", acgt(rng, 255)), ("c256", acgt(rng, 256)), ("b257", acgt(rng, 257)), ("a5000", acgt(rng, 5000))]
        seq = dict(contigs)
        refs = [("d255", 255), ("ghost", 700), ("a5000", 5000), ("e1", 1), ("b257", 257), ("c256", 256)]
        recs = []
        for n, s in contigs[1:]:
            for i in range(60 if len(s) < 1000 else 400):
                L = int(rng.integers(4, min(90, len(s) - 4) + 1))
                recs.append(read(s, f"{n}.{i}", n, int(rng.integers(2, len(s) - L - 2 + 1)), L, flag=int(rng.choice([0, 16]))))
            recs.append(read(s, f"{n}.first", n, 2, 10))                                   # the first and the last place a kept read has
            recs.append(read(s, f"{n}.last", n, len(s) - 12, 10))
            recs.append(read(s, f"{n}.pos0", n, 0, 10))                                    # position 0, the contig's end, the whole contig:
            recs.append(read(s, f"{n}.end", n, len(s) - 10, 10))                           # the tally's margin drops them
            recs.append(read(s, f"{n}.whole", n, 0, len(s)) if len(s) < 1000 else read(s, f"{n}.most", n, 2, len(s) - 4))
        recs.append(tl.Rec(qname="e1.whole", flag=0, rname="e1", pos=1, mapq=40, cigar=[(1, "M")], seq=seq["e1"], qual="I"))
        recs += [read(seq["a5000"], f"deep{i}", "a5000", 1234, 50) for i in range(300)]    # depth above 255
        recs += [read(seq["a5000"], f"lowmq{i}", "a5000", 100 + i, 30, mapq=3) for i in range(5)]
        recs += [read(seq["a5000"], f"dupflag{i}", "a5000", 200 + i, 30, flag=0x400) for i in range(5)]
        recs += [read(seq["a5000"], f"clip{i}", "a5000", 300 + i, 30, cigar=[(2, "S"), (28, "M")]) for i in range(5)]
        recs += [read("ACGT" * 40, f"ghost{i}", "ghost", 50 + i, 30) for i in range(5)]    # in the header, not in the genome
        recs += [read(seq["a5000"], f"star{i}", "*", 50 + i, 30) for i in range(3)]
        recs += [read(seq["a5000"], f"mate1.{i}", "a5000", 2000 + 7 * i, 40, flag=0x43, tlen=40) for i in range(20)]    # proper pairs: each mate
        recs += [read(seq["a5000"], f"mate2.{i}", "a5000", 2010 + 7 * i, 40, flag=0x93, tlen=-40) for i in range(20)]   # on its own, overlaps count twice
        recs += [read(seq["a5000"], f"improper{i}", "a5000", 2500 + i, 40, flag=0x41, tlen=40) for i in range(5)]
        recs += [read(seq["a5000"], f"tlen{i}", "a5000", 2600 + i, 40, flag=0x43, tlen=90) for i in range(5)]
        order = rng.permutation(len(recs))
        _CASES["small"] = Case(contigs, refs, [recs[j] for j in order], tl.PssOpts(region_len=4, min_mq=20))
    return _CASES["small"]


def long_case() -> Case:
    """one contig longer than a round of the sums scan and two tiles: the scan carries between rounds, and runs cross tile
    boundaries -- and the boundary of the round -- on a non-zero base"""
    if "long" not in _CASES:
        rng = np.random.default_rng(72)
        n = TILE * SUMS_ROUND + 2 * TILE + 77
        s = acgt(rng, n)
        recs = [read(s, f"r{i}", "big", int(p), int(L)) for i, (p, L) in enumerate(zip(rng.integers(2, n - 200, size=300), rng.integers(20, 150, size=300)))]
        edge = TILE * SUMS_ROUND - PAD                                   # the contig position at which the second round of sums begins
        recs += [read(s, f"edge{i}", "big", edge - 50 + 9 * i, 100) for i in range(8)]
        recs += [read(s, f"tile{k}.{i}", "big", TILE * k - PAD - 30 + i, 60) for k in (1, 2, 100, SUMS_ROUND + 1) for i in range(3)]
        recs += [read(s, f"wide{i}", "big", TILE * 7 - PAD - 100 + i, 2 * TILE + 300) for i in range(2)]   # over two whole tiles
        recs += [read(s, "tail", "big", n - 42, 40), read(s, "beyond", "big", n - 41, 40)]
        order = rng.permutation(len(recs))
        _CASES["long"] = Case([("big", s)], [("big", n)], [recs[j] for j in order], tl.PssOpts(region_len=4))
    return _CASES["long"]


def fuzz_case(with_rg=False, **setup) -> Case:
    key = ("fuzz", with_rg, tuple(sorted((k, str(v)) for k, v in setup.items())))
    if key not in _CASES:
        contigs, refs, recs = tl.fuzz_dataset(7201, 800, with_rg=with_rg)
        _CASES[key] = Case(contigs, refs, dl.with_copies(recs, 7201, max_copies=2), tl.PssOpts(region_len=12, min_mq=20), **setup)
    return _CASES[key]


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["KERNEL_SIMPLE", "KERNEL_TILED"])
def test_small_contigs_that_share_a_tile_and_every_category_of_read(pkg, kernel):
    c = small_case()
    got = run(pkg, c, kernel=getattr(pkg, kernel))
    want = check(c, got)
    names = [b[36:36 + b[12] - 1].decode() for b in dl.split_raw(got[4])]
    model = c.model_kept()
    assert names == [r.qname for r, k in zip(c.recs, model) if k]                       # ACGT contigs, no content filter: the candidates
    kept = set(names)
    for cat, some_kept in (("first", True), ("last", True), ("deep", True), ("mate1", True), ("mate2", True), ("most", True), ("pos0", False),
                           ("end", False), ("whole", False), ("lowmq", False), ("dupflag", False), ("clip", False), ("ghost", False), ("star", False),
                           ("improper", False), ("tlen", False)):
        members = [r.qname for r in c.recs if cat in r.qname]
        assert members and all((m in kept) == some_kept for m in members), cat        # no category is empty
    assert int(want.hist[256]) == 50 and int(want.per_contig[2][2]) >= 300                # depth above 255
    assert not want.per_contig[1].any() and not want.per_contig[3].any()                  # the ghost, the contig of one base
    assert all(want.per_contig[i][0] > 0 for i in (0, 2, 4, 5))
    assert int(want.hist.sum()) == 1 + 255 + 256 + 257 + 5000                             # padding counts nowhere
    assert int(want.per_contig[2][0]) == 4996                                             # "most" covers all a kept read can


def test_a_contig_longer_than_a_round_of_the_sums_scan(pkg):
    c = long_case()
    got = run(pkg, c)
    want = check(c, got)
    n = c.refs[0][1]
    assert n > TILE * SUMS_ROUND + 2 * TILE
    d = want.depths[0]
    edge = TILE * SUMS_ROUND - PAD
    assert d[edge - 1] > 0 and d[edge] > 0 and d[edge - 1] == d[edge]                     # a run crosses the round's boundary
    ref, st, en, dp = want.runs
    assert np.any((st < edge) & (en > edge))
    wide = slice(TILE * 7 - PAD - 99, TILE * 7 - PAD - 99 + 2 * TILE + 299)
    assert d[wide].min() > 0 and np.any(np.diff(d[wide]) != 0)                            # ... and covered stretches two whole tiles, in several runs
    assert int(d[n - 3]) == 1 and int(d[n - 2]) == 0                                      # "tail" is kept, "beyond" is not
    assert int(want.hist.sum()) == n


def test_one_block_blocks_of_one_of_seven_and_shuffled_agree(pkg):
    c = small_case()
    n = len(c.recs)
    whole = run(pkg, c)
    check(c, whole)
    for cuts in (list(range(n + 1)), list(range(0, n, 7)) + [n]):
        got = run(pkg, c, cuts=cuts)
        check(c, got)
        assert all(np.array_equal(x, y) for x, y in zip(got[:2], whole[:2])) and all(np.array_equal(x, y) for x, y in zip(got[3], whole[3]))
        assert bytes(got[4]) == bytes(whole[4])
    order = np.random.default_rng(73).permutation(n)
    shuffled = run(pkg, c, raw=tl.raw_records(c.refs, [c.recs[j] for j in order]))
    check(c, shuffled)
    assert all(np.array_equal(x, y) for x, y in zip(shuffled[:2], whole[:2])) and all(np.array_equal(x, y) for x, y in zip(shuffled[3], whole[3]))


def test_finish_twice_submit_more_finish_and_reset(pkg):
    c = small_case()
    n = len(c.recs)
    (a, oa), (b, ob) = blocks_of(pkg, c.raw, [0, n // 3, n])
    eng = c.engine(pkg)
    try:
        eng.set_coverage(True)
        eng.set_record_sink()
        c.genome(eng)
        empty = collect(eng, c)
        assert not empty[0].any() and empty[2] == 0 and int(empty[1][0]) == int(empty[1].sum()) == 5769
        eng.submit(a, oa)
        first = collect(eng, c)
        again = collect(eng, c)
        check(c, first)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1]) and first[2] == again[2]
        assert all(np.array_equal(x, y) for x, y in zip(first[3], again[3]))
        eng.submit(b, ob)
        both = collect(eng, c)
        whole = np.concatenate([first[4], both[4]])
        check(c, both, kept_raw=whole)                                                    # everything since create
        assert both[2] > first[2]
        eng.reset()
        zero = collect(eng, c)
        assert not zero[0].any() and zero[2] == 0 and len(zero[3][0]) == 0 and int(zero[1][0]) == int(zero[1].sum()) == 5769
        eng.submit(c.raw)                                                                 # the setting survived the reset
        check(c, collect(eng, c), kept_raw=whole)
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.set_coverage(False)                                                       # records have been tallied
    finally:
        eng.close()


def test_a_genome_set_again_starts_from_zero_and_runs_alone_reuse_nothing_stale(pkg):
    c = small_case()
    eng = c.engine(pkg)
    try:
        eng.set_coverage(True)
        eng.set_record_sink()
        c.genome(eng)
        eng.submit(c.raw)
        first = collect(eng, c)
        check(c, first)
        c.genome(eng)                                                                     # the same genome once more: the array is zeroed
        assert eng.finish_coverage_runs(count_only=True) == 0 and not eng.finish_coverage(len(c.refs))[0].any()
        eng.submit(c.raw)
        runs = eng.finish_coverage_runs()                                                 # the runs first, the summary behind them
        per, hist, n_runs = eng.finish_coverage(len(c.refs))
        check(c, (per, hist, n_runs, runs, eng.finish_records()))
        assert np.array_equal(per, first[0]) and all(np.array_equal(x, y) for x, y in zip(runs, first[3]))
    finally:
        eng.close()


# ---- every filter in front of it ---------------------------------------------------------------------------------------------------

def _regions(eng, c):
    names = [n for n, _ in c.refs]
    eng.set_regions(names, [0, 0, 1], [100, 900, 50], [300, 1500, 400])


COMBOS = {
    "-d": dict(before=lambda eng: eng.set_duplicates(True)),
    "-T": dict(regions=True),
    "-y": dict(read_score=dict(weights=None, min_score=40)),
    "-n": dict(mismatches=(0, 0, 0)),
    "-Q": dict(min_base_qual=25),
    "-R": dict(),
}


@pytest.mark.parametrize("combo", list(COMBOS))
def test_with_every_filter_the_coverage_is_that_of_the_sinks_records(pkg, combo):
    c = fuzz_case(with_rg=True, read_group="grpA") if combo == "-R" else fuzz_case()
    plain_case = fuzz_case(with_rg=True) if combo == "-R" else c
    kw = dict(COMBOS[combo])
    if kw.pop("regions", False):
        kw["before"] = lambda eng: _regions(eng, c)
    if "read_score" in kw:
        W = np.zeros((4, 8, 8), dtype=np.int16)
        W[1] = 100                                                                        # a C->T site is worth 100, everything else nothing
        kw["read_score"] = dict(weights=W, min_score=50)
    got = run(pkg, c, **kw)
    check(c, got)
    plain = run(pkg, plain_case)
    check(plain_case, plain)
    if combo == "-Q":                                                                     # masks bases, not reads: no effect on depth
        assert bytes(got[4]) == bytes(plain[4]) and np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    else:
        assert 0 < len(dl.split_raw(got[4])) < len(dl.split_raw(plain[4]))               # (the filter does something)
        assert int(got[0][:, 1].sum()) < int(plain[0][:, 1].sum())


# ---- the submit paths ----------------------------------------------------------------------------------------------------------------

def test_submit_device(pkg):
    c = small_case()
    want = run(pkg, c)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    offs = pkg.index_records(c.raw)
    d_r, d_o = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_r), c.raw.size + 64) == 0 and hip.hipMalloc(C.byref(d_o), offs.size * 4) == 0
    eng = c.engine(pkg)
    try:
        assert hip.hipMemcpy(d_r, c.raw.ctypes.data, c.raw.size, 1) == 0 and hip.hipMemcpy(d_o, offs.ctypes.data, offs.size * 4, 1) == 0
        eng.set_coverage(True)
        eng.set_record_sink()
        c.genome(eng)
        eng.submit_device(d_r.value, c.raw.size, d_o.value, offs.size - 1)
        got = collect(eng, c)
    finally:
        eng.close()
        hip.hipFree(d_r)
        hip.hipFree(d_o)
    check(c, got)
    assert bytes(got[4]) == bytes(want[4]) and np.array_equal(got[0], want[0])


@pytest.mark.parametrize("ahead_of_genome", [False, True])
def test_submit_bgzf(pkg, tmp_path, ahead_of_genome):
    c = fuzz_case()
    want = run(pkg, c)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, c.refs, c.recs, rng=np.random.default_rng(3))
    eng = c.engine(pkg)
    try:
        if ahead_of_genome:
            eng.feed_open(len(c.refs))
        eng.set_coverage(True, sum(ln for _, ln in c.refs))
        eng.set_record_sink()
        if not ahead_of_genome:
            c.genome(eng)
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        if ahead_of_genome:
            c.genome(eng)
        got = collect(eng, c)
        assert eng.feed_status()["flags"] == 0
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.set_coverage(False)
    finally:
        eng.close()
    check(c, got)
    assert bytes(got[4]) == bytes(want[4]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- the calls' own rules ------------------------------------------------------------------------------------------------------------

def test_count_only_calls_a_cap_that_is_too_small_and_null_pointers(pkg):
    c = small_case()
    eng = c.engine(pkg)
    L = pkg.hip_lib()
    try:
        eng.set_coverage(True)
        eng.set_record_sink()
        c.genome(eng)
        eng.submit(c.raw)
        per, hist, n_runs, runs, kept = collect(eng, c)
        want = check(c, (per, hist, n_runs, runs, kept))
        assert eng.finish_coverage_runs(count_only=True) == n_runs > 100
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage_runs(cap=n_runs - 1)
        more = eng.finish_coverage_runs(cap=n_runs + 5)                                    # more room than needed is fine
        assert all(np.array_equal(x, y) for x, y in zip(more, runs))
        # any pointer may be NULL
        n = C.c_uint64(0)
        assert L.pssbam_engine_finish_coverage(eng._h, 0, 0, None, None, 0, C.addressof(n)) == 0 and n.value == n_runs
        assert L.pssbam_engine_finish_coverage(eng._h, 0, 0, None, None, 0, None) == 0
        one = np.zeros(3, dtype=np.uint64)
        assert L.pssbam_engine_finish_coverage(eng._h, 2, 1, one.ctypes.data, None, 0, None) == 0 and np.array_equal(one, want.per_contig[2])
        small = np.zeros(3, dtype=np.uint64)                                               # a short histogram folds the rest into its last word
        assert L.pssbam_engine_finish_coverage(eng._h, 0, 0, None, small.ctypes.data, 1, None) == 0
        assert [int(v) for v in small] == [int(want.hist[0]), int(want.hist[1]), int(want.hist[2:].sum())]
        assert L.pssbam_engine_finish_coverage(eng._h, 0, 0, None, small.ctypes.data, 256, None) == -1
        assert L.pssbam_engine_finish_coverage(eng._h, 3, len(c.refs), one.ctypes.data, None, 0, None) == -1
        ends = np.zeros(n_runs, dtype=np.uint32)
        assert L.pssbam_engine_finish_coverage_runs(eng._h, n_runs, None, None, ends.ctypes.data, None, None) == 0 and np.array_equal(ends, runs[2])
    finally:
        eng.close()


def test_setter_refusals(pkg):
    kmer = pkg.Engine(kmer=dict(klen=4))
    try:
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            kmer.set_coverage(True)                          # not without the substitution tally
        kmer.set_coverage(False)                             # switching off what is off is always legal
    finally:
        kmer.close()
    eng = pkg.Engine(pss=dict(region_len=5))
    try:
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage(0)                           # the setting is off
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage_runs(count_only=True)
        eng.set_gapped(True)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_coverage(True)
        eng.set_gapped(False)
        eng.set_coverage(True)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_gapped(True)
        assert eng.finish_coverage(0)[2] == 0 and eng.finish_coverage_runs(count_only=True) == 0     # no genome yet: nothing
        eng.set_coverage(False)
        eng.set_gapped(True)                                 # off again, the two go in this order too
    finally:
        eng.close()
    c = small_case()
    eng = c.engine(pkg)
    try:
        c.genome(eng)
        eng.submit(c.raw)
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.set_coverage(True)                           # after the first submit
        eng.reset()
        eng.set_coverage(True)                               # after a reset it is legal again, with the genome there already
        eng.set_record_sink()
        eng.submit(c.raw)
        check(c, collect(eng, c))
    finally:
        eng.close()


# ---- the setting off: what the engine launched and allocated before ------------------------------------------------------------------

def test_setting_off_launches_and_counts_what_the_parent_commit_did(pkg):
    contigs, refs, recs = tl.fuzz_dataset(*OFF_INPUT)
    for mode in ("off", "toggled", "on"):
        eng = pkg.Engine(pss=dict(region_len=15))
        try:
            if mode != "off":
                eng.set_coverage(True)
            if mode == "toggled":                            # on and off again is off
                eng.set_coverage(False)
            eng.set_genome_arrays(tl.loaded_contigs(contigs))
            eng.set_references([n for n, _ in refs])
            eng.kernel_time()
            eng.submit(tl.raw_records(refs, recs))
            eng.sync()
            assert eng.kernel_time()[1] == OFF_LAUNCHES      # (on: the time and the launch count stay the tally's)
            assert eng.counters_device()[1] == OFF_N_U64
        finally:
            eng.close()

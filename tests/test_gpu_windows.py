"""Fixed windows over the depth of coverage (pssbam_engine_finish_coverage_windows) on the GPU, through the Engine wrapper.  The
expected side of every test is windows_lib, the Python restatement, over the records that the record sink of the SAME run delivers:
all seven arrays -- ref, start, end, acgt, gc, covered, depth_sum -- must be exactly equal, and the windows of a contig must sum to
its line of finish_coverage.  The cases and helpers are those of test_gpu_coverage.  Not covered: a window count beyond 32 bits (it
needs a genome of 2^36 positions) and PSSBAM_ENOMEM."""
import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

import __graft_entry__ as ge
import coverage_lib as cl
import duplicates_lib as dl
import pssbam_testlib as tl
import test_gpu_coverage as tc
import windows_lib as wl

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = tc.EINVAL, tc.ESTATE
SMALL_W = [16, 17, 255, 256, 257, 4096, 5000, 2 ** 30]
LONG_W = [16, 64, 4095, 4096, 4097, 1_000_000]       # (64: 16 514 windows, a few copies of the accumulators; 16: one; the others: 64)
EMPTY = np.zeros(0, dtype=np.uint8)


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    assert hasattr(p.hip_lib(), "pssbam_engine_finish_coverage_windows")
    return p


# ---- the data ------------------------------------------------------------------------------------------------------------------------

class RawCase(tc.Case):
    """the contigs go to the device as they are written, lower case included: the upload folds the case"""

    def loaded(self):
        if self._loaded is None:
            self._loaded = [(n, np.frombuffer(s.encode(), dtype=np.uint8).copy()) for n, s in self.contigs]
        return self._loaded


def _spice(seq: str) -> str:
    """lower case, N, IUPAC codes and runs of one base, so that acgt, gc and the window size differ; the reads keep their letters"""
    b = list(seq)

    def put(at, text):
        if 0 <= at and at + len(text) <= len(b):
            b[at:at + len(text)] = list(text)

    for at in range(5, len(b), 97):                                   # lower case all along, across every window edge
        put(at, "".join(b[at:at + 40]).lower())
    put(60, "N" * 23)
    put(100, "RYKMSWBDHVryn")
    put(130, "G" * 33)
    put(170, "a" * 20 + "T" * 15)
    put(250, "nnNN" + "c" * 9)                                        # over the edges 255, 256, 257
    for at in (1000, 2040, 3800, 4090):                               # 3840 = the tile's edge behind the genome's padding of 256
        put(at, "N" * 40 + "S" * 3 + "C" * 17 + "w" * 5)
    put(len(b) - 3, "Nn")
    return "".join(b)


_CASES: dict = {}


def small_case() -> tc.Case:
    """test_gpu_coverage's small case -- contigs of 1, 255, 256, 257 and 5000 bases in one tile, listed against the genome's order
    beside a reference the genome lacks, reads of its sixteen categories -- on contigs whose letters are spiced"""
    if "small" not in _CASES:
        c = tc.small_case()
        _CASES["small"] = RawCase([(n, _spice(s)) for n, s in c.contigs], c.refs, c.recs, c.setup.pss)
    return _CASES["small"]


def seqs_of(c) -> dict:
    return dict(c.contigs)


def want_of(c, kept_raw, W):
    return wl.from_raw(kept_raw, c.refs, seqs_of(c), W)


def check(c, eng, kept_raw, Ws, with_c=True):
    """the windows of every W against the restatement over kept_raw, and against the engine's own per-contig figures"""
    per = eng.finish_coverage(len(c.refs))[0] if with_c else None
    out = {}
    for W in Ws:
        got = eng.finish_coverage_windows(W)
        want = want_of(c, kept_raw, W)
        for name, x, y in zip(wl.NAMES, got, want):
            assert x.dtype == y.dtype and np.array_equal(x, y), (W, name, np.flatnonzero(x != y)[:8] if x.shape == y.shape else (x.shape, y.shape))
        assert eng.finish_coverage_windows(W, count_only=True) == len(want[0])
        if with_c:
            for i, (n, _) in enumerate(c.refs):
                sel = got[0] == i
                assert int(got[5][sel].sum()) == int(per[i][0]) and int(got[6][sel].astype(object).sum()) == int(per[i][1])
                if sel.any() and W >= c.lens[n]:
                    assert int(sel.sum()) == 1 and int(got[2][sel][0]) == c.lens[n]          # one window: the contig's line of -c
        out[W] = got
    return out


@contextmanager
def opened(pkg, c, raw=None, cuts=None, before=None, submit=True, **kw):
    raw = c.raw if raw is None else raw
    eng = c.engine(pkg, **kw)
    try:
        if before:
            before(eng)
        eng.set_coverage(True, sum(ln for _, ln in c.refs))
        eng.set_record_sink()
        c.genome(eng)
        if submit:
            n = pkg.index_records(raw).size - 1
            for blk, offs in tc.blocks_of(pkg, raw, cuts or [0, n]):
                eng.submit(blk, offs)
        yield eng
    finally:
        eng.close()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["KERNEL_SIMPLE", "KERNEL_TILED"])
def test_small_contigs_that_share_a_tile(pkg, kernel):
    c = small_case()
    with opened(pkg, c, kernel=getattr(pkg, kernel)) as eng:
        kept = eng.finish_records()
        got = check(c, eng, kept, SMALL_W)
    assert len(dl.split_raw(kept)) > 400                                                  # the spiced letters drop some reads, not most
    ref, start, end, acgt, gc, covered, dsum = got[16]
    size = end - start
    assert sorted(set(ref.tolist())) == [0, 2, 3, 4, 5] and len(ref) == 16 + 313 + 1 + 17 + 16    # no window for the ghost
    assert (acgt < size).any() and (acgt == 0).any() and (acgt == size).any() and (gc == acgt)[acgt > 0].any() and (gc == 0)[acgt > 0].any()
    assert (size < 16).sum() == 4 and int(size[ref == 3][0]) == 1                         # 255, 5000 % 16, 1 and 257 end short
    assert (covered == 0).any() and (covered == size).any() and ((covered > 0) & (covered < size)).any() and int(dsum.max()) > 255 * 16
    one = got[2 ** 30]
    assert len(one[0]) == 5 and one[2].tolist() == [255, 5000, 1, 257, 256]
    lower = sum(ch.islower() for _, s in c.contigs for ch in s)
    assert lower > 1000 and int(one[3].sum()) < sum(c.lens.values()) - 200                # lower case counts, N and the codes do not


def test_tile_and_round_boundaries(pkg):
    c = tc.long_case()
    n = c.refs[0][1]
    assert n == 1_056_845 and n > tc.TILE * tc.SUMS_ROUND + 2 * tc.TILE
    with opened(pkg, c) as eng:
        kept = eng.finish_records()
        got = check(c, eng, kept, LONG_W)
    ref, start, end, acgt, gc, covered, dsum = got[4097]
    assert len(ref) == -(-n // 4097) and int(end[-1]) == n and int(end[-1] - start[-1]) == n % 4097
    assert len(set((start % 16).tolist())) == 16 and len(set(((start + tc.PAD) % tc.TILE).tolist())) > 250     # edges at every offset of a lane, all over the tile
    edge = tc.TILE * tc.SUMS_ROUND - tc.PAD
    k = edge // 4097
    assert covered[k] > 0 and dsum[k] > covered[k]                                         # the window over the scan round's boundary is covered
    assert np.array_equal(acgt, end - start)                                               # (an A C G T contig)
    assert len(got[1_000_000][0]) == 2 and int(got[1_000_000][6].sum()) == int(got[16][6].sum())


# ---- the order of the calls -------------------------------------------------------------------------------------------------------------

def test_call_order_caches_more_blocks_reset_and_a_genome_set_again(pkg):
    c = small_case()
    n = len(c.recs)
    (a, oa), (b, ob) = tc.blocks_of(pkg, c.raw, [0, n // 3, n])
    same = lambda x, y: wl.same(tuple(x), tuple(y))  # noqa: E731
    with opened(pkg, c, submit=False) as eng:
        empty = eng.finish_coverage_windows(100)                                           # nothing submitted: the letters alone
        assert same(empty, want_of(c, EMPTY, 100)) and not empty[5].any() and not empty[6].any() and empty[3].any()
        eng.submit(a, oa)
        first = eng.finish_coverage_windows(100)                                           # before finish_coverage
        kept_a = eng.finish_records()
        assert same(first, want_of(c, kept_a, 100)) and first[6].any()
        per, hist, n_runs = eng.finish_coverage(len(c.refs))
        assert same(eng.finish_coverage_windows(100), first)                               # behind it
        runs = eng.finish_coverage_runs()
        assert same(eng.finish_coverage_windows(100), first)                               # behind the runs
        assert same(eng.finish_coverage_windows(100), first)                               # twice with one size,
        other = eng.finish_coverage_windows(257)                                           # another,
        assert same(other, want_of(c, kept_a, 257))
        assert same(eng.finish_coverage_windows(100), first)                               # and the first again
        tc.check(c, (per, hist, n_runs, runs, kept_a))
        again = tc.collect(eng, c)                                                         # the array and the caches are intact
        assert np.array_equal(again[0], per) and np.array_equal(again[1], hist) and again[2] == n_runs
        assert all(np.array_equal(x, y) for x, y in zip(again[3], runs))
        eng.submit(b, ob)                                                                  # more, then finish: everything since create
        both = eng.finish_coverage_windows(100)
        whole = np.concatenate([kept_a, eng.finish_records()])
        assert same(both, want_of(c, whole, 100)) and int(both[6].sum()) > int(first[6].sum())
        check(c, eng, whole, [257, 100])
        eng.reset()
        assert same(eng.finish_coverage_windows(100), empty)
        eng.submit(c.raw)                                                                  # the setting survived the reset
        assert same(eng.finish_coverage_windows(100), both)
        eng.finish_records()
        c.genome(eng)                                                                      # the same genome once more: the array is zeroed
        assert same(eng.finish_coverage_windows(100), empty)
        eng.submit(c.raw)
        assert same(eng.finish_coverage_windows(100), both)
        tc.check(c, tc.collect(eng, c), kept_raw=whole)


# ---- the submit paths ----------------------------------------------------------------------------------------------------------------

INPUT_W = [17, 256]


def test_one_block_blocks_of_one_of_seven_and_shuffled_agree(pkg):
    c = small_case()
    n = len(c.recs)
    with opened(pkg, c) as eng:
        whole = check(c, eng, eng.finish_records(), INPUT_W)
    for cuts in (list(range(n + 1)), list(range(0, n, 7)) + [n]):
        with opened(pkg, c, cuts=cuts) as eng:
            got = check(c, eng, eng.finish_records(), INPUT_W)
        assert all(wl.same(got[W], whole[W]) for W in INPUT_W)
    order = np.random.default_rng(73).permutation(n)
    with opened(pkg, c, raw=tl.raw_records(c.refs, [c.recs[j] for j in order])) as eng:
        got = check(c, eng, eng.finish_records(), INPUT_W)
    assert all(wl.same(got[W], whole[W]) for W in INPUT_W)


def test_submit_device(pkg):
    c = small_case()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    offs = pkg.index_records(c.raw)
    d_r, d_o = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_r), c.raw.size + 64) == 0 and hip.hipMalloc(C.byref(d_o), offs.size * 4) == 0
    try:
        assert hip.hipMemcpy(d_r, c.raw.ctypes.data, c.raw.size, 1) == 0 and hip.hipMemcpy(d_o, offs.ctypes.data, offs.size * 4, 1) == 0
        with opened(pkg, c, submit=False) as eng:
            eng.submit_device(d_r.value, c.raw.size, d_o.value, offs.size - 1)
            kept = eng.finish_records()
            got = check(c, eng, kept, INPUT_W)
    finally:
        hip.hipFree(d_r)
        hip.hipFree(d_o)
    assert len(dl.split_raw(kept)) > 400 and int(got[17][6].sum()) > 0


@pytest.mark.parametrize("ahead_of_genome", [False, True])
def test_submit_bgzf(pkg, tmp_path, ahead_of_genome):
    c = tc.fuzz_case()
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
        got = eng.finish_coverage_windows(100)                                             # (the call drains the feed itself)
        kept = eng.finish_records()
        assert eng.feed_status()["flags"] == 0
        assert wl.same(got, want_of(c, kept, 100)) and int(got[6].sum()) > 0
        check(c, eng, kept, [16, 1000])
    finally:
        eng.close()


def test_with_duplicate_flagging_and_a_quality_limit_in_front(pkg):
    c = tc.fuzz_case()
    with opened(pkg, c) as eng:
        plain_kept = eng.finish_records()
        plain = check(c, eng, plain_kept, [64])
    with opened(pkg, c, before=lambda e: e.set_duplicates(True), min_base_qual=25) as eng:
        kept = eng.finish_records()
        got = check(c, eng, kept, [64])
    assert 0 < len(dl.split_raw(kept)) < len(dl.split_raw(plain_kept))
    assert int(got[64][6].sum()) < int(plain[64][6].sum()) and np.array_equal(got[64][3], plain[64][3]) and np.array_equal(got[64][4], plain[64][4])


# ---- the call's own rules ------------------------------------------------------------------------------------------------------------

def test_count_only_calls_a_cap_that_is_too_small_and_null_pointers(pkg):
    c = small_case()
    L = pkg.hip_lib()
    with opened(pkg, c) as eng:
        kept = eng.finish_records()
        want = want_of(c, kept, 100)
        n = len(want[0])
        assert n == 3 + 50 + 1 + 3 + 3 and eng.finish_coverage_windows(100, count_only=True) == n
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage_windows(100, cap=n - 1)
        assert wl.same(eng.finish_coverage_windows(100, cap=n + 5), want)                  # more room than needed is fine
        cnt = C.c_uint64(0)
        f = L.pssbam_engine_finish_coverage_windows
        assert f(eng._h, 100, 0, None, None, None, None, None, None, None, C.addressof(cnt)) == 0 and cnt.value == n    # cap 0, no array: the count
        assert f(eng._h, 100, 0, None, None, None, None, None, None, None, None) == 0
        for skip in range(7):                                                              # any single array may be NULL
            arrs = [np.full(n, 0xEE, dtype=dt) for dt in wl.DTYPES]
            ptrs = [None if k == skip else a.ctypes.data for k, a in enumerate(arrs)]
            assert f(eng._h, 100, n, *ptrs, None) == 0
            assert all(k == skip or np.array_equal(a, w) for k, (a, w) in enumerate(zip(arrs, want)))
        only = np.zeros(n, dtype=np.uint64)                                                # ... and all but one
        assert f(eng._h, 100, n, None, None, None, None, None, None, only.ctypes.data, None) == 0 and np.array_equal(only, want[6])
        one = np.zeros(1, dtype=np.uint64)
        assert f(eng._h, 100, 1, None, None, None, None, None, None, one.ctypes.data, None) == -1       # a cap below the count
        for bad in (15, 0, 2 ** 30 + 1, 2 ** 32 - 1):
            with pytest.raises(pkg.PssbamError, match=EINVAL):
                eng.finish_coverage_windows(bad)
            with pytest.raises(pkg.PssbamError, match=EINVAL):
                eng.finish_coverage_windows(bad, count_only=True)
        assert wl.same(eng.finish_coverage_windows(2 ** 30), want_of(c, kept, 2 ** 30))
        assert wl.same(eng.finish_coverage_windows(100), want)                             # the refusals left the result alone


def test_refusals_by_state(pkg):
    eng = pkg.Engine(pss=dict(region_len=5))
    c = small_case()
    try:
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage_windows(100)                                               # the setting is off
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage_windows(100, count_only=True)
        eng.set_coverage(True)
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.finish_coverage_windows(100, count_only=True)                              # no genome, no references
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage_windows(15)                                                # (the size is looked at first)
        eng.set_genome_arrays(c.loaded())
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.finish_coverage_windows(100)                                               # a genome without references
        eng.set_references([n for n, _ in c.refs])
        assert wl.same(eng.finish_coverage_windows(100), want_of(c, EMPTY, 100))
        eng.set_genome_arrays(c.loaded())                                                  # a genome set again drops the references
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.finish_coverage_windows(100)
        eng.set_references([n for n, _ in c.refs][::-1])                                   # another header order: another order of windows
        back = eng.finish_coverage_windows(100)
        assert wl.same(back, wl.from_raw(EMPTY, c.refs[::-1], seqs_of(c), 100))
        eng.set_coverage(False)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_coverage_windows(100)
    finally:
        eng.close()


# ---- the call unused: what the engine launched and allocated before ---------------------------------------------------------------------

def test_call_unused_launches_and_counts_what_the_parent_commit_did(pkg):
    contigs, refs, recs = tl.fuzz_dataset(*tc.OFF_INPUT)
    for mode in ("off", "on", "on, called"):
        eng = pkg.Engine(pss=dict(region_len=15))
        try:
            if mode != "off":
                eng.set_coverage(True)
            eng.set_genome_arrays(tl.loaded_contigs(contigs))
            eng.set_references([n for n, _ in refs])
            eng.kernel_time()
            eng.submit(tl.raw_records(refs, recs))
            eng.sync()
            if mode == "on, called":                                                       # the call itself is no tally launch and counts nowhere
                assert eng.finish_coverage_windows(1000, count_only=True) > 0 and len(eng.finish_coverage_windows(1000)[0]) > 0
            assert eng.kernel_time()[1] == tc.OFF_LAUNCHES
            assert eng.counters_device()[1] == tc.OFF_N_U64
        finally:
            eng.close()

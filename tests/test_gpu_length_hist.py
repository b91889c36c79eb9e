"""pss-bam -H on the GPU: the fragment-length histogram of the reads that are added to the forward / reverse table,
counted in the tally kernel.  The yardstick is the CPU oracle's PSS_OK counter: with OK(x..y) = PSS_OK of the same
options run with -l x -L y (cut to the run's own -l / -L),
    unpaired records:                  hf[l] == hr[l] == OK(l..l)
    paired, 0x40 without 0x80:         hf[l] == OK(l..l), hr[l] == 0
    paired, 0x80 without 0x40:         the mirror image
    any input:                         hf[l] + hr[l] == 2 * OK_unpaired(l..l) + OK_paired(l..l)
and row M + 1 is the same with OK(M+1..max_read_len).  The tables and status counters must not move."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl
import regions_lib as rl

pytestmark = pytest.mark.gpu

CLASSES = ("unpaired", "first", "second", "other")


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq,
                up_ctx=o.up_ctx, down_ctx=o.down_ctx, merged_only=o.merged_only)


def flag_class(r: tl.Rec) -> str:
    if not r.flag & 0x1:
        return "unpaired"
    return {0x40: "first", 0x80: "second"}.get(r.flag & 0xC0, "other")


def split_by_flag(recs) -> dict:
    return {c: [r for r in recs if flag_class(r) == c] for c in CLASSES}


def oracle_ok_rows(oracle, g, sam: Path, o: tl.PssOpts, m: int) -> np.ndarray:
    """OK(l..l) for l = 0..m and OK(m+1..max_read_len), each cut to the run's own -l / -L"""
    out = np.zeros(m + 2, dtype=np.uint64)
    for row in range(m + 2):
        lo, hi = (row, row) if row <= m else (m + 1, o.max_read_len)
        lo, hi = max(lo, o.min_read_len), min(hi, o.max_read_len)
        if lo <= hi:
            _, _, st = oracle.pss(g, sam, tl.PssOpts(**{**pss_dict(o), "min_read_len": lo, "max_read_len": hi}))
            out[row] = st[tl.ST_OK]
    return out


class Case:
    """a record set, split by flag into SAM files, and the oracle's OK rows of every class (computed once per option set)"""

    def __init__(self, oracle, tmp: Path, contigs, refs, recs):
        self.oracle, self.contigs, self.refs, self.recs = oracle, contigs, refs, recs
        self.parts = split_by_flag(recs)
        self.sams = {}
        for c, part in self.parts.items():
            self.sams[c] = tmp / f"{c}.sam"
            tl.write_sam(self.sams[c], refs, part)
        self.g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
        self._rows = {}

    def rows(self, o: tl.PssOpts, m: int) -> dict:
        key = (tuple(sorted(pss_dict(o).items())), m)
        if key not in self._rows:
            self._rows[key] = {c: oracle_ok_rows(self.oracle, self.g, self.sams[c], o, m) for c in CLASSES}
        return self._rows[key]

    def close(self):
        self.oracle.free_genome(self.g)


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, m=0, **kw):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, length_hist=m, **kw)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if recs:
        eng.submit(tl.raw_records(refs, recs))
    return eng


def hist_of(pkg, contigs, refs, recs, o, kernel, m, **kw):
    eng = run_engine(pkg, contigs, refs, recs, o, kernel, m, **kw)
    hf, hr = eng.finish_length_hist()
    tot = eng.finish()
    eng.close()
    assert hf.shape == hr.shape == (m + 2,) and hf.dtype == np.uint64
    return hf, hr, tot


def same_but_slow_path(a, b):
    assert np.array_equal(a.fwd, b.fwd) and np.array_equal(a.rev, b.rev)
    assert {k: v for k, v in a.stats.items() if k != "slow_path"} == {k: v for k, v in b.stats.items() if k != "slow_path"}


def check_identities(pkg, case: Case, o: tl.PssOpts, kernel, m: int):
    """the per-class identities on the engine run over each subset, the sum identity on the run over all records, and
    tables + stats against an engine without the histogram"""
    want = case.rows(o, m)
    zero = np.zeros(m + 2, dtype=np.uint64)
    for c in CLASSES:
        hf, hr, _ = hist_of(pkg, case.contigs, case.refs, case.parts[c], o, kernel, m)
        if c == "unpaired":
            assert np.array_equal(hf, want[c]) and np.array_equal(hr, want[c]), (c, o)
        elif c == "first":
            assert np.array_equal(hf, want[c]) and np.array_equal(hr, zero), (c, o)
        elif c == "second":
            assert np.array_equal(hr, want[c]) and np.array_equal(hf, zero), (c, o)
        else:
            assert np.array_equal(hf + hr, want[c]), (c, o)
    hf, hr, tot = hist_of(pkg, case.contigs, case.refs, case.recs, o, kernel, m)
    paired = want["first"] + want["second"] + want["other"]
    assert np.array_equal(hf + hr, 2 * want["unpaired"] + paired), o
    assert int(hf.sum() + hr.sum()) == int(2 * want["unpaired"].sum() + paired.sum())
    plain = run_engine(pkg, case.contigs, case.refs, case.recs, o, kernel)
    same_but_slow_path(tot, plain.finish())
    plain.close()
    return hf, hr, tot


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(7301, 3000)
    case = Case(oracle, tmp_path_factory.mktemp("lenhist"), contigs, refs, recs)
    yield case
    case.close()


def fuzz_opts(n: int) -> tl.PssOpts:
    o = tl.random_pss_opts(np.random.default_rng(300 + n))
    o.region_len = n
    return o


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("n", [15, 25, 31, 40, 62])
def test_oracle_identities(pkg, fuzz, kernel, n):
    """n = 40 and 62 take two and three row passes of the tiled kernel: counting in a later pass would double the rows"""
    kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
    check_identities(pkg, fuzz, fuzz_opts(n), kern, 100)


def test_default_options_populate_every_part(pkg, fuzz):
    """the plain option set: rows below and above -r, both arrays, and the overflow row are all non-zero"""
    o = tl.PssOpts(region_len=15)
    hf, hr, _ = check_identities(pkg, fuzz, o, pkg.KERNEL_TILED, 100)
    assert not hf[:15].any() and hf[15:101].sum() > 100 and hr[15:101].sum() > 100 and hf[101] > 0 and hr[101] > 0
    assert not np.array_equal(hf, hr)


def test_overflow_path(pkg, fuzz, monkeypatch):
    """records longer than the staged prefix take the tiled kernel's one-lane path, which counts too"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    _, _, tot = check_identities(pkg, fuzz, tl.PssOpts(region_len=15), pkg.KERNEL_TILED, 100)
    assert tot.stats["slow_path"] > 0


@pytest.mark.parametrize("lds_bins", [0, 40])
def test_bins_outside_lds(pkg, fuzz, monkeypatch, lds_bins):
    """PSSBAM_HIST_LDS_BINS caps the LDS part of the arrays: every bin (0), or the bins from 40 on, take the
    wave-merged global-atomic path that limits above 1022 use for their long rows"""
    monkeypatch.setenv("PSSBAM_HIST_LDS_BINS", str(lds_bins))
    check_identities(pkg, fuzz, tl.PssOpts(region_len=15), pkg.KERNEL_TILED, 100)


# ---- one bin: the degenerate distribution ------------------------------------------------------------------------

def one_bin_data(lengths):
    rng = np.random.default_rng(5)
    ctg = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=2000))
    refs = [("clean", len(ctg))]
    recs = [tl.Rec(qname=f"c{i:06d}", flag=0, rname="clean", pos=101, mapq=30, cigar=[(ln, "M")], seq=ctg[100:100 + ln], qual="I" * ln)
            for i, ln in enumerate(lengths)]
    return [("clean", ctg)], refs, recs


@pytest.fixture(scope="module")
def one_bin():
    return one_bin_data([50] * 20000)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_one_bin(pkg, one_bin, kernel):
    contigs, refs, recs = one_bin
    kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
    hf, hr, tot = hist_of(pkg, contigs, refs, recs, tl.PssOpts(region_len=15), kern, 300)
    want = np.zeros(302, dtype=np.uint64)
    want[50] = 20000
    assert np.array_equal(hf, want) and np.array_equal(hr, want)
    assert tot.stats["pss_ok"] == 20000
    contigs, refs, recs = one_bin_data([50 + (i & 1) for i in range(20000)])
    hf, hr, _ = hist_of(pkg, contigs, refs, recs, tl.PssOpts(region_len=15), kern, 300)
    want[50] = want[51] = 10000
    assert np.array_equal(hf, want) and np.array_equal(hr, want)


@pytest.mark.parametrize("m,row", [(49, 50), (50, 50), (51, 50)])
def test_limit_around_the_length(pkg, one_bin, m, row):
    """M = 49, 50, 51 with 50 bp reads: the read lands in >M, M and M-1"""
    contigs, refs, recs = one_bin
    hf, hr, _ = hist_of(pkg, contigs, refs, recs[:3000], tl.PssOpts(region_len=15), pkg.KERNEL_TILED, m)
    want = np.zeros(m + 2, dtype=np.uint64)
    want[row] = 3000
    assert row == min(50, m + 1) and np.array_equal(hf, want) and np.array_equal(hr, want)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_largest_limit_is_the_small_one_zero_padded(pkg, fuzz, kernel):
    kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
    o = tl.PssOpts(region_len=15)
    bf, br, _ = hist_of(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, kern, 65535)
    assert bf.sum() > 500 and bf[260:].sum() == 0 and br[260:].sum() == 0   # the fuzz lengths end at 259
    for m in (300, 60):                               # 60: the rows above the limit fold into its last row
        sf, sr, _ = hist_of(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, kern, m)
        for small, big in ((sf, bf), (sr, br)):
            assert np.array_equal(big[:m + 1], small[:m + 1]) and int(big[m + 1:].sum()) == int(small[m + 1])
    assert sf[61] > 0 and sr[61] > 0


# ---- with the other filters ------------------------------------------------------------------------------------------

def sum_identity(case: Case, o, m, hf, hr):
    want = case.rows(o, m)
    assert np.array_equal(hf + hr, 2 * want["unpaired"] + want["first"] + want["second"] + want["other"])
    assert np.array_equal(hf[:m + 2] >= want["unpaired"] + want["first"], np.ones(m + 2, dtype=bool))
    assert np.array_equal(hr[:m + 2] >= want["unpaired"] + want["second"], np.ones(m + 2, dtype=bool))


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_a_read_group(pkg, oracle, tmp_path, kernel):
    contigs, refs, recs = tl.fuzz_dataset(7302, 3000, with_rg=True)
    keep = [r for r in recs if ("RG", "Z", "grpA") in r.tags]
    case = Case(oracle, tmp_path, contigs, refs, keep)
    try:
        kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
        o = tl.PssOpts(region_len=25)
        hf, hr, tot = hist_of(pkg, contigs, refs, recs, o, kern, 100, read_group="grpA")
        assert tot.stats["rg_dropped"] == len(recs) - len(keep) and hf.sum() > 100
        sum_identity(case, o, 100, hf, hr)
    finally:
        case.close()


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_regions(pkg, oracle, tmp_path, kernel):
    contigs, refs, recs, ivs = rl.fuzz_case(rl.PSS_SEEDS[0])
    case = Case(oracle, tmp_path, contigs, refs, rl.reduce_recs(recs, ivs))
    try:
        kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
        o = tl.PssOpts(region_len=15)
        eng = run_engine(pkg, contigs, refs, [], o, kern, 100)
        eng.set_regions(*rl.to_arrays(ivs))
        eng.submit(tl.raw_records(refs, recs))
        hf, hr = eng.finish_length_hist()
        eng.close()
        unfiltered, _, _ = hist_of(pkg, contigs, refs, recs, o, kern, 100)
        assert 0 < hf.sum() < unfiltered.sum()
        sum_identity(case, o, 100, hf, hr)
    finally:
        case.close()


def test_base_quality_masks_bases_not_reads(pkg, fuzz):
    o = tl.PssOpts(region_len=25)
    f0, r0, t0 = hist_of(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, pkg.KERNEL_TILED, 100)
    f20, r20, t20 = hist_of(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, pkg.KERNEL_TILED, 100, min_base_qual=20)
    assert np.array_equal(f0, f20) and np.array_equal(r0, r20) and f0.sum() > 100
    assert not np.array_equal(t0.fwd, t20.fwd)                      # the mask did bite
    plain = run_engine(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, pkg.KERNEL_TILED, min_base_qual=20)
    same_but_slow_path(t20, plain.finish())
    plain.close()


@pytest.mark.parametrize("klen", [4, 6])
def test_with_the_kmer_tally(pkg, fuzz, klen):
    """PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER (k-mer bins in LDS at k = 4, global at k = 6): histogram and k-mer tables unchanged"""
    o = tl.PssOpts(region_len=15)
    f0, r0, _ = hist_of(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, pkg.KERNEL_TILED, 100)
    res = []
    for m in (0, 100):
        eng = pkg.Engine(pss=pss_dict(o), kmer=dict(klen=klen), length_hist=m)
        eng.set_genome_arrays(tl.loaded_contigs(fuzz.contigs))
        eng.set_references([nm for nm, _ in fuzz.refs])
        eng.submit(tl.raw_records(fuzz.refs, fuzz.recs))
        res.append((eng.finish(), eng.finish_length_hist() if m else None))
        eng.close()
    (plain, _), (both, (hf, hr)) = res
    assert np.array_equal(hf, f0) and np.array_equal(hr, r0)
    assert np.array_equal(plain.k5, both.k5) and np.array_equal(plain.k3, both.k3) and plain.k5.sum() > 100
    same_but_slow_path(plain, both)
    assert plain.stats == both.stats


# ---- rules -----------------------------------------------------------------------------------------------------------

def test_rules(pkg):
    E = pkg.PssbamError
    for bad in (-1, 65536, 1 << 20):
        with pytest.raises(E):
            pkg.Engine(pss=dict(region_len=5), length_hist=bad)
    with pytest.raises(E):                                  # nothing is added to a table on a k-mer engine
        pkg.Engine(kmer=dict(klen=4), length_hist=100)
    for planes in (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]})):
        eng = pkg.Engine(pss=dict(region_len=5), **planes)
        with pytest.raises(E):                              # planes set: no histogram
            eng.set_length_histogram(100)
        assert eng.length_hist == 0
        eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), length_hist=100)
    for setter, arg in ((eng.set_read_groups, ["a"]), (eng.set_length_bins, [30]), (eng.set_contig_sets, {"x": ["chrA"]})):
        with pytest.raises(E):                              # and the other way round
            setter(arg)
    assert eng.length_hist == 100 and eng.read_groups == [] and eng.length_bins == [] and eng.contig_sets == []
    eng.set_length_histogram(0)                             # off again: the planes are legal, the arrays are gone
    with pytest.raises(E):
        eng.finish_length_hist()
    eng.set_length_bins([30])
    eng.close()

    eng = pkg.Engine(pss=dict(region_len=5), read_group="grpA", min_base_qual=10, length_hist=120)   # goes with -R and -Q
    lay = eng.counter_layout()
    assert lay["hist_fwd"] == lay["stats"] + pkg.ST_N and lay["hist_rev"] == lay["hist_fwd"] + 122
    assert lay["n_u64"] == lay["hist_rev"] + 122 == eng.counters_device()[1]
    contigs, refs, recs = tl.fuzz_dataset(5, 300, with_rg=True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    for m in (0, 60, 120):
        with pytest.raises(E):                              # records have been tallied
            eng.set_length_histogram(m)
    first = eng.finish_length_hist()
    assert first[0].sum() > 0
    eng.reset()                                             # the setting survives reset
    assert eng.counters_device()[1] == lay["n_u64"]
    zf, zr = eng.finish_length_hist()
    assert not zf.any() and not zr.any()
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_length_hist()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    eng.reset()
    eng.set_length_histogram(60)                            # legal again after reset
    assert eng.counters_device()[1] == eng.counter_layout()["n_u64"] == lay["hist_fwd"] + 2 * 62
    eng.close()

    eng = pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=3), length_hist=7)
    lay = eng.counter_layout()
    assert lay["hist_fwd"] == 2 * 7 * 16 + 2 * 64 + pkg.ST_N and lay["n_u64"] == lay["hist_fwd"] + 18 == eng.counters_device()[1]
    eng.close()

    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_length_histogram(100)
    eng.close()
    other.close()


def test_bound_counters_receive_the_histogram(pkg, fuzz):
    """a caller's block of the reported size (here: a second engine's own block) receives hf | hr at the offsets
    counter_layout() documents; read back raw, as a caller that sums blocks with RCCL would see it"""
    import ctypes as C
    o = tl.PssOpts(region_len=15)
    want_f, want_r, want = hist_of(pkg, fuzz.contigs, fuzz.refs, fuzz.recs, o, pkg.KERNEL_TILED, 100)
    eng, owner = pkg.Engine(pss=pss_dict(o), length_hist=100), pkg.Engine(pss=pss_dict(o), length_hist=100)
    lay = eng.counter_layout()
    d, n = owner.counters_device()
    assert n == lay["n_u64"] == eng.counters_device()[1]
    owner.sync()                                            # the block is zeroed
    eng.bind_counters(d, n)
    assert eng.counters_device() == (d, n)
    eng.set_genome_arrays(tl.loaded_contigs(fuzz.contigs))
    eng.set_references([nm for nm, _ in fuzz.refs])
    eng.submit(tl.raw_records(fuzz.refs, fuzz.recs))
    got = eng.finish()
    host = np.zeros(n, dtype=np.uint64)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(host.ctypes.data, d, host.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    eng.close()
    owner.close()
    assert np.array_equal(host[lay["hist_fwd"]:lay["hist_fwd"] + 102], want_f)
    assert np.array_equal(host[lay["hist_rev"]:lay["hist_rev"] + 102], want_r)
    assert np.array_equal(host[:lay["rev"]].reshape(-1, 16), want.fwd) and np.array_equal(got.fwd, want.fwd)
    assert int(host[lay["stats"] + pkg.ST_NAMES.index("pss_ok")]) == want.stats["pss_ok"]


def test_submit_bgzf_histogram_set_after_feed_open(pkg, oracle, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(7303, 4000)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    case = Case(oracle, tmp_path, contigs, refs, recs)
    try:
        o = tl.PssOpts(region_len=15, min_mq=5)
        eng = pkg.Engine(pss=pss_dict(o))
        eng.feed_open(len(refs))
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        eng.set_length_histogram(100)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        hf, hr = eng.finish_length_hist()
        sum_identity(case, o, 100, hf, hr)
        ref_f, ref_r, ref_tot = hist_of(pkg, contigs, refs, recs, o, pkg.KERNEL_TILED, 100)
        assert np.array_equal(hf, ref_f) and np.array_equal(hr, ref_r) and hf.sum() > 100
        assert eng.feed_status()["flags"] == 0
        tot = eng.finish()
        assert tot.stats["records"] == len(recs)
        same_but_slow_path(tot, ref_tot)
        eng.close()
    finally:
        case.close()


# ---- the command line ----------------------------------------------------------------------------------------------

CLI_MODES = {
    "bam_device_feed": ("bam", {}),
    "bam_host_reader": ("bam", {"PSSBAM_DEVICE_INFLATE": "0"}),
    "sam": ("sam", {}),
    "bam_two_gpus": ("bam", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}),
}
CLI_M = 120
CLI_LENGTHS = (25, 40, 60, 88, 120)


def parse_lengths(path: Path, fa: Path, aln: Path, m: int):
    lines = path.read_bytes().decode().split("\n")
    assert lines[:4] == ["# fragment lengths of the reads added to the forward / reverse table", f"# FASTA: {fa}", f"# BAM: {aln}",
                         "length\tfwd\trev"]
    assert lines[-1] == "" and len(lines) == 4 + m + 2 + 1
    rows = [ln.split("\t") for ln in lines[4:-1]]
    assert [r[0] for r in rows] == [str(k) for k in range(m + 1)] + [f">{m}"] and all(len(r) == 3 for r in rows)
    return np.array([int(r[1]) for r in rows], dtype=np.uint64), np.array([int(r[2]) for r in rows], dtype=np.uint64)


@pytest.fixture(scope="module")
def cli_case(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(7304, 6000)
    case = Case(oracle, tmp_path_factory.mktemp("lenhist_cli"), contigs, refs, tl.ref_safe(recs))
    yield case
    case.close()


def write_aln(path: Path, fmt: str, refs, recs):
    if fmt == "bam":
        tl.write_bam(path, refs, recs, rng=np.random.default_rng(2))
    else:
        tl.write_sam(path, refs, recs)


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_H(pkg, cli_case, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    case = cli_case
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, case.contigs)
    aln = tmp_path / f"in.{fmt}"
    write_aln(aln, fmt, case.refs, case.recs)
    o = tl.PssOpts(region_len=25, min_mq=10)
    env = {**os.environ, **extra}
    prefix = tmp_path / "out"

    def run(aln_path, out, opts, *more, stats=False):
        return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln_path), "-o", str(out), *more] + opts.argv(), capture_output=True,
                              text=True, env={**env, "PSSBAM_STATS": "1"} if stats else env, timeout=300)

    pr = run(aln, prefix, o, "-H", str(CLI_M))
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(f" -H {CLI_M}")
    assert sorted(p.name for p in tmp_path.glob("out.*")) == ["out.pss.counts.txt", "out.pss.lengths.txt", "out.pss.rates.txt"]
    counts, rates = Path(f"{prefix}.pss.counts.txt").read_bytes(), Path(f"{prefix}.pss.rates.txt").read_bytes()
    hf, hr = parse_lengths(Path(f"{prefix}.pss.lengths.txt"), fa, aln, CLI_M)
    # counts and rates: byte-identical to the same command without -H, which writes no lengths file
    plain = tmp_path / "plain"
    pr = run(aln, plain, o)
    assert pr.returncode == 0, pr.stderr
    assert Path(f"{plain}.pss.counts.txt").read_bytes().replace(b"plain.pss", b"out.pss") == counts
    assert Path(f"{plain}.pss.rates.txt").read_bytes().replace(b"plain.pss", b"out.pss") == rates
    assert not Path(f"{plain}.pss.lengths.txt").exists()
    # every row through the oracle identities on the flag-split files
    want = case.rows(o, CLI_M)
    assert np.array_equal(hf + hr, 2 * want["unpaired"] + want["first"] + want["second"] + want["other"])
    assert hf[25:121].sum() > 300 and hf[121] > 0 and not hf[:25].any()
    parts = {}
    for c in ("unpaired", "first", "second"):
        part_aln = tmp_path / f"{c}.{fmt}"
        write_aln(part_aln, fmt, case.refs, case.parts[c])
        pr = run(part_aln, tmp_path / c, o, "-H", str(CLI_M))
        assert pr.returncode == 0, pr.stderr
        parts[c] = (part_aln, *parse_lengths(tmp_path / f"{c}.pss.lengths.txt", fa, part_aln, CLI_M))
    zero = np.zeros(CLI_M + 2, dtype=np.uint64)
    assert np.array_equal(parts["unpaired"][1], want["unpaired"]) and np.array_equal(parts["unpaired"][2], want["unpaired"])
    assert np.array_equal(parts["first"][1], want["first"]) and np.array_equal(parts["first"][2], zero)
    assert np.array_equal(parts["second"][2], want["second"]) and np.array_equal(parts["second"][1], zero)
    # the unpaired subset against this binary's own -l x -L x runs
    for ln in CLI_LENGTHS:
        ol = tl.PssOpts(**{**pss_dict(o), "min_read_len": ln, "max_read_len": ln})
        pr = run(parts["unpaired"][0], tmp_path / "one", ol, stats=True)
        assert pr.returncode == 0, pr.stderr
        ok = [int(x.split("=")[1]) for x in pr.stderr.splitlines() if x.startswith("[pssbam] pss_ok=")]
        assert ok == [int(parts["unpaired"][1][ln])] == [int(parts["unpaired"][2][ln])], ln
    pr = run(aln, tmp_path / "bad", o, "-H", str(CLI_M), "-G")
    assert pr.returncode == 1 and "-H" in pr.stderr and "-G" in pr.stderr and "exclude each other" in pr.stderr
    assert not list(tmp_path.glob("bad.*"))

    if tl.have_ref() and mode in ("bam_device_feed", "sam"):
        # ACGT-only input, -r 1: every read added to the forward table adds exactly one count to row 2 of the
        # reference's forward table, so hf[l] is that row's sum from the reference run with -l l -L l
        clean = lambda s: "".join(ch if ch in "ACGTacgt" else "A" for ch in s)   # noqa: E731
        fa2 = tmp_path / "acgt.fa"
        tl.write_fasta(fa2, [(nm, clean(s)) for nm, s in case.contigs])
        recs2 = [tl.Rec(**{**r.__dict__, "seq": clean(r.seq)}) for r in case.recs if r.seq != "*"]
        aln2 = tmp_path / f"acgt.{fmt}"
        write_aln(aln2, fmt, case.refs, recs2)
        o1 = tl.PssOpts(region_len=1, min_mq=10)
        pr = subprocess.run([str(exe), "-F", str(fa2), "-B", str(aln2), "-o", str(tmp_path / "acgt"), "-H", str(CLI_M)] + o1.argv(),
                            capture_output=True, text=True, env=env, timeout=300)
        assert pr.returncode == 0, pr.stderr
        af, _ = parse_lengths(tmp_path / "acgt.pss.lengths.txt", fa2, aln2, CLI_M)
        for ln in CLI_LENGTHS:
            ol = tl.PssOpts(**{**pss_dict(o1), "min_read_len": ln, "max_read_len": ln})
            rf, _, _, _, _ = tl.run_ref_pss(fa2, aln2, tmp_path / f"ref{ln}", ol, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
            assert int(rf[2].sum()) == int(af[ln]), ln
        assert sum(int(af[ln]) for ln in CLI_LENGTHS) > 0

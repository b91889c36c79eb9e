"""pss-bam -E on the GPU: a second pair of tables, COND, over the unpaired reads whose OTHER end carries a given
substitution within its first d positions, and four read counters, from the same pass as the ordinary tables T.

The specification is end_condition_lib's: COND.fwd == the forward table of the tool without -E on the input reduced to
the unpaired 3'-marked records, COND.rev == the reverse table on the input reduced to the 5'-marked ones, reads[] == its
PSS_OK on the unpaired / 5'-marked / 3'-marked / both-marked records.  So every check here runs the engine (or the
command) with the setting on the ORIGINAL records and compares with the CPU oracle without it on the reduced copies
(checked on their own in test_end_condition_host.py); T and the status counters are compared with the same engine
without the setting."""
import ctypes as C
import os
import subprocess
from dataclasses import replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import end_condition_lib as ec
import pssbam_testlib as tl
import regions_lib as rl
from test_gpu_length_hist import CLI_MODES, pss_dict, write_aln

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
KERNELS = ["SIMPLE", "TILED", "AUTO"]
SS, DS = (13, 13), (13, 2)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def kern_of(pkg, kernel):
    return {"SIMPLE": pkg.KERNEL_SIMPLE, "TILED": pkg.KERNEL_TILED, "AUTO": pkg.KERNEL_AUTO}[kernel]


def make_engine(pkg, contigs, refs, o: tl.PssOpts, kernel, cond, **kw):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_group=o.read_group, end_condition=cond, **kw)
    assert eng.end_condition == cond
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    return eng


def run_both(pkg, contigs, refs, recs, o, kernel, cond, regions=None, **kw):
    """(T, (fwd_c, rev_c, reads)) of an engine with the setting, after checking T and the status counters against the
    same engine without it"""
    out = []
    for c in (cond, None):
        eng = make_engine(pkg, contigs, refs, o, kernel, c, **kw)
        if regions is not None:
            eng.set_regions(*rl.to_arrays(regions))
        if len(recs):
            eng.submit(tl.raw_records(refs, recs))
        fin = eng.finish_end_condition() if c else None
        out.append((eng.finish(), fin))
        eng.close()
    (tot, fin), (plain, _) = out
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev)
    assert tot.stats == plain.stats
    return tot, fin


def check(fin, want, ctx=""):
    for k, name in enumerate(("COND.fwd", "COND.rev", "reads")):
        assert np.array_equal(fin[k], want[k]), (name, ctx, fin[2], want[2])


def oracle_expected(oracle, tmp, contigs, refs, recs, o, cond, min_bq=0, mask=None):
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        return ec.expected(oracle, g, tmp, refs, contigs, recs, o, *cond, min_bq=min_bq, mask=mask)
    finally:
        oracle.free_genome(g)


# ---- fuzz --------------------------------------------------------------------------------------------------------------

FUZZ_SEED = 8101
FUZZ_N = [1, 2, 7, 15, 16, 17, 28, 30, 15, 30, 7, 28]
FUZZ_CELLS = [SS, DS, (0, 0), None, SS, DS, (0, 15), None, (5, 10), SS, DS, None]     # None: a random pair of cells
ANY_CELLS = [0, 2, 5, 10, 13, 15]                   # the matches and the two transitions that deamination makes


def fuzz_draws():
    """one draw per entry of FUZZ_N: (options, (depth, cell5, cell3)); -q -l -L -m -U -D at random"""
    rng = np.random.default_rng(FUZZ_SEED)
    ctx = ["ACGT", "ACGT", "ACGT", "CT", "ACGTN", "TA", "GY", "AG"]
    draws = []
    for n, cells in zip(FUZZ_N, FUZZ_CELLS):
        o = tl.PssOpts(region_len=n, min_read_len=int(rng.choice([0, 0, 10, 25])), max_read_len=int(rng.choice([250000000, 250000000, 60, 120])),
                       min_mq=int(rng.choice([0, 0, 0, 20])), up_ctx=str(rng.choice(ctx)), down_ctx=str(rng.choice(ctx)),
                       merged_only=bool(rng.random() < 0.3))
        d = min(int(rng.choice([1, 2, 3, 8])), n)
        if cells is None:
            cells = (int(rng.choice(ANY_CELLS)), int(rng.choice(ANY_CELLS)))
        draws.append((o, (d, *cells)))
    return draws


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    """about 2000 records of the testlib's generator with terminal damage planted, and the expectation of every draw"""
    contigs, refs, recs = tl.fuzz_dataset(FUZZ_SEED, 2000)
    recs = ec.plant_damage(contigs, recs, np.random.default_rng(FUZZ_SEED + 1), 0.5)
    tmp = tmp_path_factory.mktemp("endc")
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    want = [ec.expected(oracle, g, tmp, refs, contigs, recs, o, *cond) for o, cond in fuzz_draws()]
    oracle.free_genome(g)
    return contigs, refs, recs, want


@pytest.mark.parametrize("kernel", KERNELS)
def test_fuzz(pkg, fuzz, kernel):
    contigs, refs, recs, want = fuzz
    skipped = 0
    for (o, cond), w in zip(fuzz_draws(), want):
        if min(int(w[2][1]), int(w[2][2])) < 10:            # fewer than 10 records in either COND table
            skipped += 1
            continue
        tot, fin = run_both(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), cond)
        check(fin, w, (kernel, o, cond))
    assert skipped * 5 <= len(FUZZ_N), skipped
    both = [int(w[2][3]) for (o, cond), w in zip(fuzz_draws(), want)]
    assert max(both) >= 20                                  # both-marked reads are common in some draw


# ---- a swept mark ---------------------------------------------------------------------------------------------------------

SWEEP_L = 40


def sweep_case(low_qual=False):
    """One clean read per strand, end and k = 0..9 with the one cell TC (read T on reference C, read orientation) at
    position k from that end, each on a contig of its own that is all A but for the one base.  `low_qual`: the planted
    base has quality 5, every other base 40."""
    contigs, recs, where = [], [], []
    for is_rev in (False, True):
        for end5 in (True, False):
            for k in range(10):
                at_left = end5 != is_rev                    # the 5' end of a reverse-strand read is the right alignment end
                p = k if at_left else SWEEP_L - 1 - k
                name = f"c{len(contigs):02d}"
                ref = ["A"] * (SWEEP_L + 8)
                ref[4 + p] = "G" if is_rev else "C"
                seq = ["A"] * SWEEP_L
                seq[p] = "A" if is_rev else "T"             # complemented: T on C
                qual = ["I"] * SWEEP_L
                if low_qual:
                    qual[p] = chr(33 + 5)
                contigs.append((name, "".join(ref)))
                recs.append(tl.Rec(f"s{len(recs):03d}", 16 if is_rev else 0, name, 5, 30, [(SWEEP_L, "M")], seq="".join(seq), qual="".join(qual)))
                where.append((end5, k))
    return contigs, [(n, len(s)) for n, s in contigs], recs, where


@pytest.mark.parametrize("kernel", KERNELS)
def test_swept_mark(pkg, oracle, kernel, tmp_path):
    """marked exactly when k < d: off-by-ones in the even / odd split of the code words and in the mirrored right window"""
    contigs, refs, recs, where = sweep_case()
    o = tl.PssOpts(region_len=12)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    for d in range(1, 9):
        m5 = [r for r, (end5, k) in zip(recs, where) if end5 and k < d]
        m3 = [r for r, (end5, k) in zip(recs, where) if not end5 and k < d]
        tl.write_sam(tmp_path / "m5.sam", refs, m5)
        tl.write_sam(tmp_path / "m3.sam", refs, m3)
        want = (oracle.pss(g, tmp_path / "m3.sam", o)[0], oracle.pss(g, tmp_path / "m5.sam", o)[1], np.array([40, 2 * d, 2 * d, 0], dtype=np.uint64))
        tot, fin = run_both(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), (d, *SS))
        check(fin, want, (kernel, d))
        assert tot.stats["pss_ok"] == 40 and int(fin[0][0].sum()) == 2 * d
        # the marks themselves agree with the yardstick's
        assert [ec.marks(contigs, r, d, *SS) for r in recs] == [(end5 and k < d, (not end5) and k < d) for end5, k in where]
    oracle.free_genome(g)


@pytest.mark.parametrize("kernel", KERNELS)
def test_low_quality_mark_does_not_mark(pkg, kernel):
    contigs, refs, recs, where = sweep_case(low_qual=True)
    o = tl.PssOpts(region_len=12)
    tot, fin = run_both(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), (8, *SS), min_base_qual=20)
    assert list(fin[2]) == [40, 0, 0, 0] and not fin[0].any() and not fin[1].any()
    tot, fin = run_both(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), (8, *SS), min_base_qual=5)
    assert list(fin[2]) == [40, 16, 16, 0]


# ---- short reads --------------------------------------------------------------------------------------------------------

def clean_reads(seed, lengths, per_len=12, sub=0.25):
    """unpaired <L>M reads of the given lengths on one random A/C/G/T contig, both strands, every base substituted with
    probability `sub`"""
    rng = np.random.default_rng(seed)
    ctg = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=600))
    recs = []
    for L in lengths:
        for _ in range(per_len):
            s = int(rng.integers(2, len(ctg) - L - 2))
            seq = "".join("ACGT"[int(rng.integers(0, 4))] if rng.random() < sub else b for b in ctg[s:s + L])
            recs.append(tl.Rec(f"q{len(recs):05d}", 16 * int(rng.integers(0, 2)), "ctg", s + 1, 30, [(L, "M")], seq=seq, qual="I" * L))
    return [("ctg", ctg)], [("ctg", len(ctg))], recs


SHORT = [("L == region_len", 15, 3, [15], (0, 15)), ("windows overlap at -r 1", 1, 1, range(1, 41), (5, 10)),
         ("L < 2d", 8, 8, range(8, 16), (13, 2)), ("L < 2d, match cells", 8, 8, range(8, 16), (0, 0))]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("what,n,d,lengths,cells", SHORT, ids=[s[0] for s in SHORT])
def test_short_reads(pkg, oracle, kernel, what, n, d, lengths, cells, tmp_path):
    contigs, refs, recs = clean_reads(31 + n, list(lengths), per_len=40 if len(list(lengths)) == 1 else 12)
    o = tl.PssOpts(region_len=n)
    want = oracle_expected(oracle, tmp_path, contigs, refs, recs, o, (d, *cells))
    tot, fin = run_both(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), (d, *cells))
    check(fin, want, (kernel, what))
    assert want[2][1] >= 5 and want[2][2] >= 5 and want[2][0] == tot.stats["pss_ok"]


# ---- paired records ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_paired_records_never_reach_cond(pkg, fuzz, kernel):
    contigs, refs, recs, _ = fuzz
    paired = [r for r in recs if r.flag & 1]
    tot, fin = run_both(pkg, contigs, refs, paired, tl.PssOpts(region_len=15), kern_of(pkg, kernel), (3, 0, 0))
    assert tot.stats["pss_ok"] > 20 and tot.fwd.sum() > 100 and tot.rev.sum() > 100
    assert not fin[0].any() and not fin[1].any() and not fin[2].any()


# ---- -Q, regions, -R -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_with_min_base_quality(pkg, oracle, fuzz, kernel, tmp_path):
    """a base below q has no cell: it neither marks nor counts"""
    contigs, refs, recs, _ = fuzz
    for n, cond in ((15, (2, *SS)), (30, (8, 0, 15))):
        o = tl.PssOpts(region_len=n)
        want = oracle_expected(oracle, tmp_path, contigs, refs, recs, o, cond, min_bq=20, mask=lambda part: bq.mask_recs(part, 20))
        plain = oracle_expected(oracle, tmp_path, contigs, refs, recs, o, cond)
        tot, fin = run_both(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), cond, min_base_qual=20)
        check(fin, want, (kernel, n))
        assert want[2][1] >= 10 and want[2][2] >= 10 and want[2][1] < plain[2][1]      # -Q did take marks away


@pytest.mark.parametrize("kernel", KERNELS)
def test_with_regions_and_read_group(pkg, oracle, kernel, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(8102, 3000, with_rg=True)
    recs = ec.plant_damage(contigs, recs, np.random.default_rng(5), 0.6)
    ivs = rl.fuzz_intervals(8102, contigs, recs)
    kept = [r for r in rl.reduce_recs(recs, ivs) if ("RG", "Z", "grpA") in r.tags]
    o = tl.PssOpts(region_len=15)
    cond = (3, *DS)
    want = oracle_expected(oracle, tmp_path, contigs, refs, kept, o, cond, min_bq=15, mask=lambda part: bq.mask_recs(part, 15))
    tot, fin = run_both(pkg, contigs, refs, recs, replace(o, read_group="grpA"), kern_of(pkg, kernel), cond, regions=ivs, min_base_qual=15)
    check(fin, want, kernel)
    assert want[2][1] >= 5 and want[2][2] >= 5 and tot.stats["rg_dropped"] > 100


# ---- the one-lane path ---------------------------------------------------------------------------------------------------

def test_overflow_path(pkg, oracle, tmp_path, monkeypatch):
    """records whose needed prefix exceeds what is staged (long names, aux data) take the one-lane path: same tables"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    contigs, refs, recs = tl.fuzz_dataset(8103, 2000, with_rg=True, extras=True)
    recs = ec.plant_damage(contigs, recs, np.random.default_rng(6), 0.6)
    for n, cond, q in ((15, (1, *SS), 0), (28, (3, 0, 0), 0), (15, (2, *DS), 20)):
        o = tl.PssOpts(region_len=n)
        want = oracle_expected(oracle, tmp_path, contigs, refs, recs, o, cond, min_bq=q, mask=(lambda part: bq.mask_recs(part, q)) if q else None)
        tot, fin = run_both(pkg, contigs, refs, recs, o, pkg.KERNEL_TILED, cond, min_base_qual=q)
        assert tot.stats["slow_path"] > 0
        check(fin, want, (n, cond, q))
        assert want[2][1] >= 5


# ---- block shapes ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_block_shapes(pkg, oracle, kernel, tmp_path):
    contigs, refs, recs = clean_reads(77, [20, 33, 50, 64], per_len=1300, sub=0.2)
    o = tl.PssOpts(region_len=15)
    cond = (2, 0, 15)
    kern = kern_of(pkg, kernel)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    wants = {}
    for count in (1, 31, 33, 129, len(recs)):
        wants[count] = ec.expected(oracle, g, tmp_path, refs, contigs, recs[:count], o, *cond)
        tot, fin = run_both(pkg, contigs, refs, recs[:count], o, kern, cond)
        check(fin, wants[count], (kernel, count))
    oracle.free_genome(g)
    assert wants[len(recs)][2][3] > 50
    eng = make_engine(pkg, contigs, refs, o, kern, cond)
    eng.submit(tl.raw_records(refs, recs[:129]))
    eng.submit(tl.raw_records(refs, recs))                  # two submits accumulate
    fin = eng.finish_end_condition()
    check(fin, tuple(wants[129][k] + wants[len(recs)][k] for k in range(3)), (kernel, "two submits"))
    eng.reset()
    fin = eng.finish_end_condition()
    assert not fin[0].any() and not fin[1].any() and not fin[2].any()
    eng.submit(tl.raw_records(refs, recs[:33]))             # the setting survives reset
    check(eng.finish_end_condition(), wants[33], (kernel, "after reset"))
    eng.close()


# ---- rules ---------------------------------------------------------------------------------------------------------------

def test_rules(pkg):
    E = pkg.PssbamError
    eng = pkg.Engine(pss=dict(region_len=5))
    plain_n = eng.counters_device()[1]
    for bad in ((-1, 13, 13), (9, 13, 13), (1, -1, 13), (1, 16, 13), (1, 13, -1), (1, 13, 16), (6, 13, 13)):
        with pytest.raises(E):                              # out of range; depth > region_len
            eng.set_end_condition(*bad)
    with pytest.raises(E):                                  # off: nothing to finish
        eng.finish_end_condition()
    eng.set_end_condition(0, 13, 13)                        # off stays off
    assert eng.end_condition is None and eng.counters_device()[1] == plain_n == eng.counter_layout()["n_u64"]
    eng.set_end_condition(5, 13, 2)
    assert eng.end_condition == (5, 13, 2) and eng.counters_device()[1] == plain_n + 2 * 7 * 16 + 4
    eng.set_end_condition(0)
    assert eng.counters_device()[1] == plain_n
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=31))
    with pytest.raises(E):                                  # region_len > 30
        eng.set_end_condition(1, 13, 13)
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=30), end_condition=(8, 13, 13))
    eng.close()
    for cfg in (dict(kmer=dict(klen=4)), dict(pss=dict(region_len=5), kmer=dict(klen=4))):
        with pytest.raises(E):                              # PSSBAM_TALLY_KMER in the mask
            pkg.Engine(end_condition=(1, 13, 13), **cfg)
    for other in (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]}), dict(length_hist=100),
                  dict(site_context="cpg")):
        eng = pkg.Engine(pss=dict(region_len=5), **other)
        with pytest.raises(E):                              # planes, histogram or site context set: no end condition
            eng.set_end_condition(1, 13, 13)
        assert eng.end_condition is None
        eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), end_condition=(1, 13, 13))
    for setter, arg in ((eng.set_read_groups, ["a"]), (eng.set_length_bins, [30]), (eng.set_contig_sets, {"x": ["chrA"]}),
                        (eng.set_length_histogram, 100), (eng.set_site_context, "cpg")):
        with pytest.raises(E):                              # and the other way round
            setter(arg)
    assert eng.end_condition == (1, 13, 13) and eng.read_groups == [] and eng.length_bins == [] and eng.contig_sets == []
    assert eng.length_hist == 0 and eng.site_context is None
    eng.set_end_condition(0)                                # off again: the planes are legal, the pair is gone
    with pytest.raises(E):
        eng.finish_end_condition()
    eng.set_length_bins([30])
    eng.close()

    eng = pkg.Engine(pss=dict(region_len=5), read_group="grpA", min_base_qual=10, end_condition=(2, 13, 13))   # goes with -R and -Q
    lay = eng.counter_layout()
    assert lay["end_fwd"] == lay["stats"] + pkg.ST_N == 2 * 7 * 16 + pkg.ST_N and lay["end_rev"] == lay["end_fwd"] + 7 * 16
    assert lay["end_reads"] == lay["end_rev"] + 7 * 16 and lay["n_u64"] == lay["end_reads"] + 4 == eng.counters_device()[1]
    contigs, refs, recs = tl.fuzz_dataset(5, 300, with_rg=True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    for args in ((2, 13, 13), (1, 13, 13), (0, 0, 0)):
        with pytest.raises(E):                              # records have been tallied
            eng.set_end_condition(*args)
    eng.reset()                                             # the setting survives reset; legal again after it
    assert eng.counters_device()[1] == lay["n_u64"] and eng.end_condition == (2, 13, 13)
    eng.set_end_condition(0)
    assert eng.counters_device()[1] == eng.counter_layout()["n_u64"] == lay["end_fwd"]
    eng.close()

    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_end_condition(1, 13, 13)
    eng.close()
    other.close()


def test_depth_zero_is_the_untouched_engine(pkg, fuzz):
    contigs, refs, recs, _ = fuzz
    o = tl.PssOpts(region_len=15)
    blocks = []
    for touch in (False, True):
        eng = pkg.Engine(pss=pss_dict(o))
        if touch:
            eng.set_end_condition(3, 13, 2)
            eng.set_end_condition(0, 13, 2)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        eng.submit(tl.raw_records(refs, recs))
        eng.sync()
        d, n = eng.counters_device()
        blocks.append(device_words(d, n))
        eng.close()
    assert blocks[0].size == blocks[1].size == 2 * 17 * 16 + 16 and np.array_equal(blocks[0], blocks[1]) and blocks[0].any()


# ---- the counter block -------------------------------------------------------------------------------------------------

def device_words(d: int, n: int) -> np.ndarray:
    host = np.zeros(n, dtype=np.uint64)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(host.ctypes.data, d, host.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    return host


def test_bound_torch_tensor_receives_the_block(pkg, oracle, fuzz, tmp_path):
    """a torch tensor of the reported size receives [fwd | rev | stats | fwd_c | rev_c | reads] at the documented offsets"""
    import torch
    contigs, refs, recs, _ = fuzz
    o = tl.PssOpts(region_len=28)
    cond = (3, 0, 0)
    want = oracle_expected(oracle, tmp_path, contigs, refs, recs, o, cond)
    eng = pkg.Engine(pss=pss_dict(o), end_condition=cond)
    lay = eng.counter_layout()
    n = eng.counters_device()[1]
    assert n == lay["n_u64"] == 2 * 30 * 16 + 16 + 2 * 30 * 16 + 4
    block = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.bind_counters(block.data_ptr(), n)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    tot = eng.finish()
    fin = eng.finish_end_condition()
    host = block.cpu().numpy().astype(np.uint64)
    eng.close()
    cells = 30 * 16
    assert np.array_equal(host[lay["end_fwd"]:lay["end_fwd"] + cells].reshape(-1, 16), want[0])
    assert np.array_equal(host[lay["end_rev"]:lay["end_rev"] + cells].reshape(-1, 16), want[1])
    assert np.array_equal(host[lay["end_reads"]:lay["end_reads"] + 4], want[2]) and want[2][3] >= 20
    assert np.array_equal(host[:cells].reshape(-1, 16), tot.fwd) and int(host[lay["stats"] + pkg.ST_NAMES.index("pss_ok")]) == tot.stats["pss_ok"]
    check(fin, want)


def test_two_engines_reduce_to_the_concatenated_run(pkg, oracle, fuzz, tmp_path):
    contigs, refs, recs, _ = fuzz
    o = tl.PssOpts(region_len=15)
    cond = (2, *SS)
    want = oracle_expected(oracle, tmp_path, contigs, refs, recs, o, cond)
    half = len(recs) // 2
    engs = [make_engine(pkg, contigs, refs, o, pkg.KERNEL_AUTO, cond) for _ in range(2)]
    engs[0].submit(tl.raw_records(refs, recs[:half]))
    engs[1].submit(tl.raw_records(refs, recs[half:]))
    L = pkg.hip_lib()
    arr = (C.c_void_p * 2)(engs[0]._h, engs[1]._h)
    assert L.pssbam_reduce_counters(arr, 2, 0) == 0
    fin, tot = engs[0].finish_end_condition(), engs[0].finish()
    whole = make_engine(pkg, contigs, refs, o, pkg.KERNEL_AUTO, None)
    whole.submit(tl.raw_records(refs, recs))
    plain = whole.finish()
    for e in engs + [whole]:
        e.close()
    check(fin, want)
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev) and tot.stats["pss_ok"] == plain.stats["pss_ok"]
    assert want[2][1] >= 10


# ---- the command line ----------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


CLI_CASES = {"ss": ["-E", "ss"], "ds": ["-E", "ds"], "ss3": ["-E", "ss,3"], "ss_q20": ["-E", "ss", "-Q", "20"]}


@pytest.mark.parametrize("mode", list(CLI_MODES))
@pytest.mark.parametrize("case", list(CLI_CASES))
def test_cli_reproduces_the_goldens(pkg, mode, case, tmp_path):
    """bin/pss-bam -E on setD writes the committed cond files byte for byte (but for the lines that name files) on every
    input route, and the ordinary two files as without -E"""
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    env = {**os.environ, **extra}
    aln = GOLD / ("setD.bam" if fmt == "bam" else "setD.sam")
    args = CLI_CASES[case]
    plain_args = args[2:]

    def run(out, more):
        return subprocess.run([str(exe), "-F", str(GOLD / "setD.fa"), "-B", str(aln), "-o", str(out), *more], capture_output=True,
                              env=env, timeout=300)

    pr = run(tmp_path / "out", args)
    assert pr.returncode == 0, pr.stderr
    assert f" -E {args[1]}" in pr.stderr.decode().splitlines()[0]
    assert sorted(p.name for p in tmp_path.glob("out.*")) == sorted(
        [f"out.pss.{k}.txt" for k in ("counts", "rates")] + [f"out.cond.pss.{k}.txt" for k in ("counts", "rates", "reads")])
    pr = run(tmp_path / "plain", plain_args)
    assert pr.returncode == 0, pr.stderr
    for kind in ("counts", "rates"):
        assert (tmp_path / f"plain.pss.{kind}.txt").read_bytes().replace(b"plain.pss", b"out.pss") == (tmp_path / f"out.pss.{kind}.txt").read_bytes()
        got = (tmp_path / f"out.cond.pss.{kind}.txt").read_text()
        assert f"out.cond.pss.{kind}.txt" in [ln for ln in got.splitlines() if ln.startswith("### OUT")][0]
        assert report_body(got) == report_body((GOLD / f"cond_{case}_setD.pss.{kind}.txt").read_text()), kind
    assert (tmp_path / "out.cond.pss.reads.txt").read_text() == (GOLD / f"cond_{case}_setD.pss.reads.txt").read_text()


@pytest.mark.parametrize("args", [["-E", "ss", "-G"], ["-E", "ss", "-S", "40"], ["-E", "ds", "-H", "100"], ["-E", "ds", "-X", "cpg"],
                                  ["-E", "ss", "-r", "31"]])
def test_cli_refusals_exit_1(pkg, args, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(GOLD / "setD.fa"), "-B", str(GOLD / "setD.sam"), "-o", str(tmp_path / "out"), *args],
                        capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "-E" in pr.stderr and list(tmp_path.iterdir()) == []

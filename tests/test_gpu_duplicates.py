"""Duplicate flagging (pssbam_engine_set_duplicates) on the GPU, through the Engine wrapper.  The feature's definition is an
identity: a run with the setting on equals the run without it on the same records after the duplicates -- as duplicates_lib, the
Python restatement, names them -- have had FLAG 0x400 set.  So the expected side of every test is the same engine without the
setting on the model-flagged records: tables, planes, every status counter and the sinks' bytes must be bit-identical, and the
totals and the group-size histogram must be the model's."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import __graft_entry__ as ge
import duplicates_lib as dl
import pssbam_testlib as tl
import read_score_lib as rs

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = "pssbam error -1:", "pssbam error -5:"
# the figures of the commit before the setting existed, for OFF_INPUT with the setting off: pssbam_engine_kernel_time's launch count
# and the counter block's words
OFF_INPUT = (7, 3000)     # tl.fuzz_dataset(seed, n_reads), one submit, pss region_len 15
OFF_LAUNCHES, OFF_N_U64 = 1, 560


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    assert hasattr(p.hip_lib(), "pssbam_engine_set_duplicates")
    return p


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq, up_ctx=o.up_ctx,
                down_ctx=o.down_ctx, merged_only=o.merged_only)


def fk_dict(o: tl.FkOpts) -> dict:
    return dict(klen=o.klen, min_mq=o.min_mq, min_read_len=o.min_read_len, max_read_len=o.max_read_len, merged_only=o.merged_only)


class Case:
    """a genome, a header, records, and what eligibility depends on; the model's verdict and the flagged records, once"""

    def __init__(self, contigs, refs, recs, **setup):
        self.contigs, self.refs, self.recs = contigs, refs, recs
        self.setup = dl.Setup(refs, {n: len(s) for n, s in contigs}, **setup)
        self.raw = tl.raw_records(refs, recs)
        self.verdict = dl.judge_recs(recs, self.setup)
        self.flagged = dl.flag_raw(self.raw, self.verdict.dup)

    def engine(self, pkg, **kw):
        s = self.setup
        eng = pkg.Engine(pss=pss_dict(s.pss) if s.pss else None, kmer=fk_dict(s.fk) if s.fk else None, read_group=s.read_group,
                         read_groups=s.groups, **kw)
        return eng

    def genome(self, eng):
        eng.set_genome_arrays(tl.loaded_contigs(self.contigs))
        eng.set_references([n for n, _ in self.refs])


def blocks_of(pkg, raw, cuts):
    """raw cut at the record indices `cuts` -> [(bytes, offsets)]"""
    offs = pkg.index_records(raw)
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            o = offs[a:b + 1].astype(np.int64)
            out.append((raw[o[0]:o[-1]], (o - o[0]).astype(np.uint32)))
    return out


def run(pkg, c: Case, raw, dedup, cuts=None, slots=0, sink=False, **kw):
    """-> dict(tabs, groups, totals, hist, kept, launches)"""
    eng = c.engine(pkg, **kw)
    try:
        if dedup:
            eng.set_duplicates(True, slots)
        if sink:
            eng.set_record_sink()
        c.genome(eng)
        eng.kernel_time()
        n = pkg.index_records(raw).size - 1
        for blk, offs in blocks_of(pkg, raw, cuts or [0, n]):
            eng.submit(blk, offs)
        return collect(eng, c, dedup, sink)
    finally:
        eng.close()


def collect(eng, c: Case, dedup, sink=False):
    out = dict(kept=eng.finish_records() if sink else None)
    out["launches"] = eng.kernel_time()[1]
    out["tabs"] = eng.finish()
    out["groups"] = eng.finish_groups() if c.setup.groups else None
    out["totals"], out["hist"] = eng.finish_duplicates() if dedup else (None, None)
    return out


def same_tables(a, b):
    for x, y in ((a.fwd, b.fwd), (a.rev, b.rev), (a.k5, b.k5), (a.k3, b.k3)):
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y)):
            return False
    return a.stats == b.stats


def check(got, want, c: Case, verdict=None):
    v = verdict or c.verdict
    assert same_tables(got["tabs"], want["tabs"]), (got["tabs"].stats, want["tabs"].stats)
    assert got["launches"] == want["launches"]
    if want["groups"] is not None:
        assert got["groups"].keys() == want["groups"].keys()
        for k in want["groups"]:
            assert same_tables(got["groups"][k], want["groups"][k]), k
    if want["kept"] is not None:
        assert bytes(got["kept"]) == bytes(want["kept"])
    assert got["totals"] == v.totals
    assert np.array_equal(got["hist"], v.hist)


def acgt_contig(rng, n) -> str:
    """upper-case A C G T only: every candidate read on it passes the default -U / -D contexts"""
    return "".join("ACGT"[int(v)] for v in rng.integers(0, 4, size=n))


_FUZZ: dict = {}


def fuzz_case(seed, region_len=15, n=800, **setup) -> Case:
    key = (seed, region_len, n, tuple(sorted((k, str(v)) for k, v in setup.items())))
    if key not in _FUZZ:
        contigs, refs, recs = tl.fuzz_dataset(seed, n, with_rg=bool(setup.get("groups") or setup.get("read_group")))
        if "fk" not in setup:
            setup["pss"] = tl.PssOpts(region_len=region_len, min_mq=20)
        _FUZZ[key] = Case(contigs, refs, dl.with_copies(recs, seed), **setup)
    return _FUZZ[key]


# ---- identity on fuzz data ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("region_len", [15, 40])
@pytest.mark.parametrize("kernel", ["KERNEL_SIMPLE", "KERNEL_TILED"])
def test_identity_on_fuzz_data_with_injected_copies(pkg, kernel, region_len):
    """each record repeated 0..5 times; -r 15 takes tally_compact, -r 40 two passes of tally_tiled"""
    c = fuzz_case(6101, region_len)
    assert c.verdict.totals["flagged"] > 300 and int(c.verdict.hist[6]) > 0
    k = getattr(pkg, kernel)
    got, want = run(pkg, c, c.raw, True, kernel=k), run(pkg, c, c.flagged, False, kernel=k)
    check(got, want, c)
    plain = run(pkg, c, c.raw, False, kernel=k)
    assert plain["tabs"].stats["pss_ok"] > got["tabs"].stats["pss_ok"] > 0      # (the setting does something)
    assert got["tabs"].stats["pss_filtered"] - plain["tabs"].stats["pss_filtered"] == plain["tabs"].stats["pss_ok"] - got["tabs"].stats["pss_ok"]


def test_two_runs_give_identical_results(pkg):
    c = fuzz_case(6101)
    a, b = run(pkg, c, c.raw, True), run(pkg, c, c.raw, True)
    assert same_tables(a["tabs"], b["tabs"]) and a["totals"] == b["totals"] and np.array_equal(a["hist"], b["hist"])


# ---- same (refID, POS), different rest: the two-word key ---------------------------------------------------------------------------

def one_position_case(n_refs):
    rng = np.random.default_rng(62)
    contigs = [(f"c{k}", acgt_contig(rng, 600)) for k in range(n_refs)]
    refs = [(n, len(s)) for n, s in contigs]
    recs = []
    for i in range(4096):
        L, rev, k = 20 + i % 64, (i // 64) % 2, (i // 128) % n_refs
        recs.append(tl.Rec(qname=f"r{i}", flag=0x10 if rev else 0, rname=f"c{k}", pos=101, mapq=40, cigar=[(L, "M")],
                           seq=contigs[k][1][100:100 + L], qual="".join(chr(33 + int(q)) for q in rng.integers(2, 42, size=L))))
    return Case(contigs, refs, recs, pss=tl.PssOpts(region_len=10))


@pytest.mark.parametrize("n_refs", [1, 2])
def test_4096_records_at_one_position_64_lengths_both_strands(pkg, n_refs):
    """every key shares word a (refID << 32 | POS) with 127 others: a slot whose a is claimed may get its b from a rival"""
    c = one_position_case(n_refs)
    assert c.verdict.totals == {"eligible": 4096, "distinct": 128 * n_refs, "flagged": 4096 - 128 * n_refs}
    got, want = run(pkg, c, c.raw, True, sink=True), run(pkg, c, c.flagged, False, sink=True)
    check(got, want, c)
    assert got["tabs"].stats["pss_ok"] == 128 * n_refs
    assert got["totals"]["distinct"] == 128 * n_refs and int(got["hist"][4096 // (128 * n_refs)]) == 128 * n_refs


# ---- independence of the block cuts, reset ------------------------------------------------------------------------------------------

def test_block_cuts_do_not_matter(pkg):
    c = fuzz_case(6102, n=220)
    n = len(c.recs)
    first_dup = int(np.flatnonzero(c.verdict.dup)[0])      # a cut right in front of a duplicate is a cut inside its group
    whole = run(pkg, c, c.raw, True, sink=True)
    check(whole, run(pkg, c, c.flagged, False, sink=True), c)
    for cuts in (list(range(n + 1)), list(range(0, n, 7)) + [n], [0, first_dup, n]):
        got = run(pkg, c, c.raw, True, cuts=cuts, sink=True)
        assert same_tables(got["tabs"], whole["tabs"]) and got["totals"] == whole["totals"] and np.array_equal(got["hist"], whole["hist"])
        assert bytes(got["kept"]) == bytes(whole["kept"])


def test_reset_empties_the_table_and_keeps_the_setting(pkg):
    c = fuzz_case(6102, n=220)
    eng = c.engine(pkg)
    try:
        eng.set_duplicates(True)
        c.genome(eng)
        eng.submit(c.raw)
        first = collect(eng, c, True)
        eng.reset()
        empty = eng.finish_duplicates()
        assert empty[0] == {"eligible": 0, "distinct": 0, "flagged": 0} and not empty[1].any()
        eng.submit(c.raw)                                    # (a table that still held the first run would flag every eligible record)
        second = collect(eng, c, True)
        assert same_tables(first["tabs"], second["tabs"]) and first["totals"] == second["totals"] == c.verdict.totals
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.set_duplicates(False)                        # records have been tallied
    finally:
        eng.close()


# ---- unsorted input: the first in input order wins ---------------------------------------------------------------------------------

def test_shuffled_input_keeps_the_first_of_each_group(pkg):
    contigs, refs, recs = tl.fuzz_dataset(6103, 500)
    c = Case(contigs, refs, dl.with_copies(recs, 6103, shuffle=True), pss=tl.PssOpts(region_len=12, min_mq=20))
    got, want = run(pkg, c, c.raw, True, sink=True), run(pkg, c, c.flagged, False, sink=True)
    check(got, want, c)
    kept = {b[36:36 + b[12] - 1].decode() for b in dl.split_raw(got["kept"])}
    idx = {n: i for i, (n, _) in enumerate(refs)}
    firsts, later = set(), set()
    seen = set()
    for r, el, d in zip(c.recs, c.verdict.eligible, c.verdict.dup):
        if el:
            (later if d else firsts).add(r.qname)
            assert d == (dl.key_of(dl.core_of_rec(r, idx), c.setup) in seen)
            seen.add(dl.key_of(dl.core_of_rec(r, idx), c.setup))
    assert len(later) > 200 and not (kept & later) and kept <= firsts | {r.qname for r in c.recs if r.flag & 1}
    assert len(kept & firsts) > 50


# ---- growth ---------------------------------------------------------------------------------------------------------------------------

def test_growth_from_16_slots_over_several_blocks(pkg):
    rng = np.random.default_rng(64)
    contigs = [("g", acgt_contig(rng, 3000))]
    refs, recs = [("g", 3000)], []
    for i in range(5000):
        pos0, L = 3 + i // 2, 30 + i % 2
        recs.append(tl.Rec(qname=f"k{i}", flag=0, rname="g", pos=pos0 + 1, mapq=30, cigar=[(L, "M")], seq=contigs[0][1][pos0:pos0 + L], qual="I" * L))
    recs += [replace(r, qname=r.qname + "d") for r in recs[::3]]
    order = rng.permutation(len(recs))
    c = Case(contigs, refs, [recs[j] for j in order], pss=tl.PssOpts(region_len=8))
    assert c.verdict.totals == {"eligible": 6667, "distinct": 5000, "flagged": 1667}
    cuts = list(range(0, len(recs), 1300)) + [len(recs)]
    small, default = run(pkg, c, c.raw, True, cuts=cuts, slots=16), run(pkg, c, c.raw, True, cuts=cuts)
    want = run(pkg, c, c.flagged, False, cuts=cuts)
    check(small, want, c)
    check(default, want, c)


# ---- what does not shadow -----------------------------------------------------------------------------------------------------------

def test_an_ineligible_first_member_does_not_shadow_the_rest(pkg):
    rng = np.random.default_rng(65)
    contigs = [("c", acgt_contig(rng, 1000))]
    refs = [("c", 1000)]
    seq = contigs[0][1][100:130]
    mk = lambda name, **kw: tl.Rec(**{**dict(qname=name, flag=0, rname="c", pos=101, mapq=40, cigar=[(30, "M")], seq=seq, qual="I" * 30), **kw})  # noqa: E731
    recs = [mk("lowmq", mapq=3), mk("secondary", flag=0x100), mk("clipped", cigar=[(2, "S"), (28, "M")]), mk("flagged", flag=0x400),
            mk("paired", flag=0x43, tlen=30), mk("first"), mk("dup1"), mk("paired2", flag=0x83, tlen=30), mk("dup2")]
    c = Case(contigs, refs, recs, pss=tl.PssOpts(region_len=5, min_mq=30))
    assert [r.qname for r, d in zip(recs, c.verdict.dup) if d] == ["dup1", "dup2"]
    got, want = run(pkg, c, c.raw, True, sink=True), run(pkg, c, c.flagged, False, sink=True)
    check(got, want, c)
    assert [b[36:36 + b[12] - 1].decode() for b in dl.split_raw(got["kept"])] == ["paired", "first", "paired2"]


def test_read_groups_are_part_of_the_key_and_R_of_eligibility(pkg):
    grouped = fuzz_case(6106, 12, groups=["grpA", "grpB"])
    assert grouped.verdict.totals["flagged"] > 300
    check(run(pkg, grouped, grouped.raw, True), run(pkg, grouped, grouped.flagged, False), grouped)
    ungrouped = dl.judge_recs(grouped.recs, replace(grouped.setup, groups=None))
    assert ungrouped.totals["distinct"] <= grouped.verdict.totals["distinct"]
    only = fuzz_case(6106, 12, read_group="grpA")
    assert 100 < only.verdict.totals["eligible"] < grouped.verdict.totals["eligible"]
    check(run(pkg, only, only.raw, True), run(pkg, only, only.flagged, False), only)
    # the same coordinates in two groups are two keys; another group's record does not shadow under -R
    rng = np.random.default_rng(66)
    contigs = [("c", acgt_contig(rng, 500))]
    mk = lambda name, rg: tl.Rec(qname=name, flag=0, rname="c", pos=51, mapq=40, cigar=[(25, "M")], seq=contigs[0][1][50:75], qual="I" * 25,  # noqa: E731
                                 tags=[("RG", "Z", rg)])
    recs = [mk("a1", "A"), mk("b1", "B"), mk("a2", "A"), mk("b2", "B")]
    two = Case(contigs, [("c", 500)], recs, pss=tl.PssOpts(region_len=5), groups=["A", "B"])
    got = run(pkg, two, two.raw, True)
    check(got, run(pkg, two, two.flagged, False), two)
    assert got["totals"] == {"eligible": 4, "distinct": 2, "flagged": 2} and got["tabs"].stats["pss_ok"] == 2
    under_r = Case(contigs, [("c", 500)], recs, pss=tl.PssOpts(region_len=5), read_group="B")
    got = run(pkg, under_r, under_r.raw, True)
    check(got, run(pkg, under_r, under_r.flagged, False), under_r)
    assert got["totals"] == {"eligible": 2, "distinct": 1, "flagged": 1} and got["tabs"].stats["pss_ok"] == 1


def test_content_filters_come_after_deduplication(pkg):
    """the first of a group scores low, the second high: under a score filter nothing of the group is tallied or kept"""
    contigs = [("c", "ACGT" * 10 + "AACCCCCCCCCCTTGGAATTAATTGGAATTAAGG" + "ACGT" * 10)]
    refs = [("c", len(contigs[0][1]))]
    ref = contigs[0][1][40:70]
    damaged = ref.replace("C", "T", 3)
    W = np.zeros((4, 8, 8), dtype=np.int16)
    W[1] = 100                                              # a C->T site is worth 100, everything else nothing
    mk = lambda name, seq, **kw: tl.Rec(**{**dict(qname=name, flag=0, rname="c", pos=41, mapq=40, cigar=[(30, "M")], seq=seq, qual="I" * 30), **kw})  # noqa: E731
    recs = [mk("clean", ref), mk("damaged", damaged), mk("alone", damaged, pos=43)]
    assert [rs.score(r, contigs, W) for r in recs] == [0, 300, 300]
    c = Case(contigs, refs, recs, pss=tl.PssOpts(region_len=5))
    score = dict(weights=W, min_score=50)
    got = run(pkg, c, c.raw, True, sink=True, read_score=score)
    check(got, run(pkg, c, c.flagged, False, sink=True, read_score=score), c)
    assert [b[36:36 + b[12] - 1].decode() for b in dl.split_raw(got["kept"])] == ["alone"] and got["tabs"].stats["pss_ok"] == 1
    assert run(pkg, c, c.raw, False, sink=True, read_score=score)["tabs"].stats["pss_ok"] == 2   # (without the setting "damaged" is tallied)


# ---- the submit paths ----------------------------------------------------------------------------------------------------------------

def test_submit_device_flags_the_callers_buffer_at_the_models_records(pkg):
    c = fuzz_case(6101)
    want = run(pkg, c, c.flagged, False)
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
        eng.set_duplicates(True)
        c.genome(eng)
        eng.kernel_time()
        eng.submit_device(d_r.value, c.raw.size, d_o.value, offs.size - 1)
        got = collect(eng, c, True)
        back = np.zeros_like(c.raw)
        assert hip.hipMemcpy(back.ctypes.data, d_r, c.raw.size, 2) == 0
    finally:
        eng.close()
        hip.hipFree(d_r)
        hip.hipFree(d_o)
    check(got, want, c)
    assert bytes(back) == bytes(c.flagged) and bytes(back) != bytes(c.raw)


@pytest.mark.parametrize("ahead_of_genome", [False, True])
def test_submit_bgzf(pkg, tmp_path, ahead_of_genome):
    c = fuzz_case(6101)
    want = run(pkg, c, c.flagged, False)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, c.refs, c.recs, rng=np.random.default_rng(3))
    eng = c.engine(pkg)
    try:
        if ahead_of_genome:
            eng.feed_open(len(c.refs))
        eng.set_duplicates(True)
        if not ahead_of_genome:
            c.genome(eng)
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        if ahead_of_genome:
            c.genome(eng)
        tabs = eng.finish()
        totals, hist = eng.finish_duplicates()
        assert eng.feed_status()["flags"] == 0
    finally:
        eng.close()
    assert same_tables(tabs, want["tabs"]) and totals == c.verdict.totals and np.array_equal(hist, c.verdict.hist)


# ---- the k-mer engine, and what the setter refuses -----------------------------------------------------------------------------------

def test_kmer_engine_identity(pkg):
    c = fuzz_case(6107, fk=tl.FkOpts(klen=4, min_mq=10, min_read_len=5, max_read_len=200))
    assert c.verdict.totals["flagged"] > 500
    got, want = run(pkg, c, c.raw, True), run(pkg, c, c.flagged, False)
    check(got, want, c)
    assert got["tabs"].stats["kmer_filtered"] > run(pkg, c, c.raw, False)["tabs"].stats["kmer_filtered"]


def test_setter_refusals(pkg):
    both = pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4))
    try:
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            both.set_duplicates(True)
        both.set_duplicates(False)                           # switching off what is off is always legal
    finally:
        both.close()
    eng = pkg.Engine(pss=dict(region_len=5))
    try:
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_duplicates()                          # the setting is off
        eng.set_gapped(True)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_duplicates(True)
        eng.set_gapped(False)
        eng.set_duplicates(True)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_gapped(True)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_duplicates(hist_max=65536)
        assert eng.finish_duplicates(hist_max=0)[0] == {"eligible": 0, "distinct": 0, "flagged": 0}
    finally:
        eng.close()


# ---- the setting off: what the engine launched and allocated before ------------------------------------------------------------------

def test_setting_off_launches_and_counts_what_the_parent_commit_did(pkg):
    contigs, refs, recs = tl.fuzz_dataset(*OFF_INPUT)
    for toggled in (False, True):
        eng = pkg.Engine(pss=dict(region_len=15))
        try:
            if toggled:                                      # on and off again is off
                eng.set_duplicates(True)
                eng.set_duplicates(False)
            eng.set_genome_arrays(tl.loaded_contigs(contigs))
            eng.set_references([n for n, _ in refs])
            eng.kernel_time()
            eng.submit(tl.raw_records(refs, recs))
            eng.sync()
            assert eng.kernel_time()[1] == OFF_LAUNCHES
            assert eng.counters_device()[1] == OFF_N_U64
        finally:
            eng.close()
    # ... and with the setting on the tally's launch count and the counter block are still those
    eng = pkg.Engine(pss=dict(region_len=15))
    try:
        eng.set_duplicates(True)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([n for n, _ in refs])
        eng.kernel_time()
        eng.submit(tl.raw_records(refs, recs))
        eng.sync()
        assert eng.kernel_time()[1] == OFF_LAUNCHES and eng.counters_device()[1] == OFF_N_U64
    finally:
        eng.close()

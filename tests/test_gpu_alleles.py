"""Strand-split allele counts at listed sites (pssbam_engine_set_sites) on the GPU, through the Engine wrapper.  The expected side of
every test is alleles_lib, the Python restatement, over the records that the record sink of the SAME run delivers: the resolved
sites, their reference letters, the ten counters of each and the totals must be exactly equal."""
import numpy as np
import pytest

import __graft_entry__ as ge
import alleles_lib as al
import duplicates_lib as dl
import pssbam_testlib as tl
import test_gpu_coverage as tgc
from test_gpu_coverage import Case, acgt, blocks_of, read

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = "pssbam error -1:", "pssbam error -5:"
SHIFTS = (2, 10, 20)              # PSSBAM_SITE_GRID_SHIFT: the smallest, the default, the largest


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    assert hasattr(p.hip_lib(), "pssbam_engine_set_sites")
    return p


def send(eng, sites, trim=0):
    names = sorted({n for n, _ in sites})
    at = {n: k for k, n in enumerate(names)}
    eng.set_sites(names, [at[n] for n, _ in sites], [p for _, p in sites], trim)


def check(c: Case, got, kept, sites, trim=0, min_bq=0):
    """got = Engine.finish_sites(); kept = the sink's records the counts are of"""
    ref, pos0, base, counts, totals = got
    res, want = al.from_raw(kept, c.refs, c.lens, sites, trim, min_bq)
    assert ref.dtype == np.int32 and pos0.dtype == np.uint32 and counts.dtype == np.uint32 and counts.shape == (ref.size, 10)
    assert np.array_equal(ref, res.ref) and np.array_equal(pos0, res.pos0)
    assert np.array_equal(base, al.ref_bases(res, c.refs, dict(c.contigs)))
    assert np.array_equal(counts, want), np.argwhere(counts != want)[:5]
    assert totals == al.totals(res, want)
    return res, want


def run(pkg, c: Case, sites, trim=0, raw=None, cuts=None, before=None, sites_after_refs=False, **kw):
    raw = c.raw if raw is None else raw
    eng = c.engine(pkg, **kw)
    try:
        if before:
            before(eng)
        if not sites_after_refs:
            send(eng, sites, trim)
        eng.set_record_sink()
        c.genome(eng)
        if sites_after_refs:
            send(eng, sites, trim)
        eng.kernel_time()
        n = pkg.index_records(raw).size - 1
        for blk, offs in blocks_of(pkg, raw, cuts or [0, n]):
            eng.submit(blk, offs)
        return eng.finish_sites(), eng.finish_records()
    finally:
        eng.close()


# ---- the site lists ------------------------------------------------------------------------------------------------------------------

def site_list(c: Case, kind: str) -> list:
    every = [(n, p) for n, ln in c.lens.items() for p in range(ln)]
    if kind == "every":
        return every + [("ghost", p) for p in range(0, 700, 7)]
    if kind == "one":
        return [("a5000", 1250)]
    if kind == "margins":
        return [(n, p) for n, ln in c.lens.items() for p in sorted({0, 1, 2, ln - 3, ln - 2, ln - 1}) if 0 <= p < ln]
    if kind == "ghost_and_beyond":
        return ([("ghost", 60), ("ghost", 0), ("nowhere", 5)] + [(n, ln + d) for n, ln in c.lens.items() for d in (0, 1, 1000)] +
                [("a5000", 2 ** 32 - 1), ("a5000", 1234), ("c256", 255), ("c256", 256)])
    if kind == "duplicates_unsorted":
        rng = np.random.default_rng(75)
        some = [every[j] for j in rng.integers(0, len(every), size=900)]
        return some + some[::3] + [("a5000", 1250)] * 4
    raise KeyError(kind)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind", ["every", "one", "margins", "ghost_and_beyond", "duplicates_unsorted"])
def test_site_lists_at_every_grid_shift(pkg, monkeypatch, kind, shift):
    monkeypatch.setenv("PSSBAM_SITE_GRID_SHIFT", str(shift))
    c = tgc.small_case()
    sites = site_list(c, kind)
    got, kept = run(pkg, c, sites)
    res, want = check(c, got, kept, sites)
    if kind == "every":
        assert res.ref.size == 5769 and got[4]["given"] == 5769 + 100 and int(want.sum()) == sum(al.read_of_raw(b).L for b in dl.split_raw(kept))
        assert int(want.astype(np.int64).sum(axis=1).max()) >= 300 and all(int(want[:, k].sum()) > 0 for k in (0, 1, 2, 3, 5, 6, 7, 8))
    if kind == "one":
        assert res.ref.size == 1 and int(want.sum()) >= 300
    if kind == "margins":
        sums = want.astype(np.int64).sum(axis=1)
        edge = np.array([p < 2 or p >= c.lens[c.refs[int(r)][0]] - 2 for r, p in zip(res.ref, res.pos0)])
        assert edge.any() and not sums[edge].any() and sums[~edge].any()                  # a kept read never reaches the outer two
    if kind == "ghost_and_beyond":
        assert [(c.refs[int(r)][0], int(p)) for r, p in zip(res.ref, res.pos0)] == [("a5000", 1234), ("c256", 255)]
    if kind == "duplicates_unsorted":
        assert got[4]["given"] == res.ref.size == len(set(sites)) < len(sites)


# ---- the reads -----------------------------------------------------------------------------------------------------------------------

_CASES: dict = {}


def q(*vals) -> str:
    return "".join(chr(33 + v) for v in vals)


def reads_case() -> Case:
    """one contig; reads at even and odd starts with even and odd lengths on both strands, N and IUPAC letters in SEQ, qualities on
    both sides of 20, one-base reads without QUAL, and pairs whose SEQ is shorter (and longer) than their CIGAR"""
    if "reads" not in _CASES:
        rng = np.random.default_rng(76)
        s = acgt(rng, 700)
        recs = []
        for start in (10, 11, 40, 41):
            for L in (12, 13):
                for flag in (0, 16):
                    recs.append(read(s, f"par.{start}.{L}.{flag}", "c", start, L, flag=flag))
        iupac = "NACMGRSVTWYHKDBN="
        recs.append(read(s, "iupac.f", "c", 100, len(iupac), seq=iupac))
        recs.append(read(s, "iupac.r", "c", 103, len(iupac), seq=iupac[::-1], flag=16))
        for i in range(60):
            L = int(rng.integers(8, 40))
            p = int(rng.integers(2, 600))
            seq = "".join(rng.choice(list("ACGTN"), size=L, p=[.22, .22, .22, .22, .12]))
            recs.append(read(s, f"mixq.{i}", "c", p, L, seq=seq, qual=q(*rng.choice([0, 5, 19, 20, 21, 40], size=L)), flag=int(rng.choice([0, 16]))))
        for i in range(6):
            recs.append(tl.Rec(qname=f"noqual.{i}", flag=16 * (i & 1), rname="c", pos=300 + i, mapq=40, cigar=[(1, "M")], seq=s[299 + i], qual="*"))
        for i in range(6):                                                                 # SEQ of 30 or 31 under a 40M CIGAR, TLEN 40
            n = 30 + (i & 1)
            recs.append(read(s, f"short.{i}", "c", 400 + 3 * i, 40, seq=s[400 + 3 * i:400 + 3 * i + n], qual=q(*([30] * n)), flag=0x43 if i < 3 else 0x93,
                             tlen=40 if i < 3 else -40))
        for i in range(2):                                                                 # ... and one that is longer
            recs.append(read(s, f"long.{i}", "c", 500 + i, 20, seq=s[500 + i:530 + i], qual=q(*([30] * 30)), flag=0x43, tlen=20))
        order = rng.permutation(len(recs))
        _CASES["reads"] = Case([("c", s)], [("c", 700)], [recs[j] for j in order], tl.PssOpts(region_len=1))
    return _CASES["reads"]


@pytest.mark.parametrize("min_bq", [0, 20])
def test_nibble_parity_strands_iupac_qualities_absent_qual_and_a_seq_shorter_than_its_cigar(pkg, min_bq):
    c = reads_case()
    sites = [("c", p) for p in range(700)]
    got, kept = run(pkg, c, sites, **({"min_base_qual": min_bq} if min_bq else {}))
    res, want = check(c, got, kept, sites, min_bq=min_bq)
    names = {b[36:36 + b[12] - 1].decode().split(".")[0] for b in dl.split_raw(kept)}
    assert names == {"par", "iupac", "mixq", "noqual", "short", "long"}                    # every category has kept reads
    assert len(dl.split_raw(kept)) == len(c.recs)
    other = int(want[:, 4].sum()) + int(want[:, 9].sum())
    if min_bq == 0:
        _CASES["other_plain"] = other
        assert other >= 2 * 13 + 6 * 9                                                     # IUPAC and N letters, the offsets beyond l_seq
    else:
        assert other > _CASES.get("other_plain", 0) and int(want.sum()) == sum(al.read_of_raw(b).L for b in dl.split_raw(kept))
    at = {int(p): k for k, p in enumerate(res.pos0)}
    for i in range(6):                                                                     # absent QUAL is never below the minimum
        row = want[at[299 + i]]
        assert int(row[(5 if i & 1 else 0) + "ACGT".index(dict(c.contigs)["c"][299 + i])]) >= 1


def test_five_thousand_reads_over_one_site(pkg):
    if "hot" not in _CASES:
        rng = np.random.default_rng(77)
        s = acgt(rng, 300)
        recs = []
        for i in range(5000):
            p = int(rng.integers(52, 100))
            seq = list(s[p:p + 50])
            seq[100 - p] = "ACGTN"[int(rng.integers(0, 5))]
            recs.append(read(s, f"h{i}", "hot", p, 50, seq="".join(seq), flag=int(rng.choice([0, 16]))))
        _CASES["hot"] = Case([("hot", s)], [("hot", 300)], recs, tl.PssOpts(region_len=4))
    c = _CASES["hot"]
    sites = [("hot", 100)]
    got, kept = run(pkg, c, sites)
    _, want = check(c, got, kept, sites)
    assert int(want.sum()) == 5000 and int(want.min()) > 300                               # every one of the ten counters, under contention
    got7, kept7 = run(pkg, c, sites, cuts=list(range(0, 5000, 713)) + [5000])
    assert np.array_equal(got7[3], got[3]) and bytes(kept7) == bytes(kept)


@pytest.mark.parametrize("trim", [0, 1, 15, 16, 65535])
def test_trim(pkg, trim):
    """reads of 31 bases: 16 = L/2 rounded up leaves nothing, 15 the middle base alone"""
    if "uniform" not in _CASES:
        rng = np.random.default_rng(78)
        s = acgt(rng, 900)
        recs = [read(s, f"u{i}", "u", int(p), 31, flag=int(f)) for i, (p, f) in enumerate(zip(rng.integers(2, 860, size=400), rng.choice([0, 16], size=400)))]
        _CASES["uniform"] = Case([("u", s)], [("u", 900)], recs, tl.PssOpts(region_len=4))
    c = _CASES["uniform"]
    sites = [("u", p) for p in range(900)]
    got, kept = run(pkg, c, sites, trim=trim)
    _, want = check(c, got, kept, sites, trim=trim)
    assert len(dl.split_raw(kept)) == 400
    assert int(want.sum()) == 400 * max(31 - 2 * trim, 0) and got[4]["bases"] == int(want.sum())
    small, kept_s = run(pkg, tgc.small_case(), site_list(tgc.small_case(), "every"), trim=trim)       # lengths on both sides of 2 * trim
    check(tgc.small_case(), small, kept_s, site_list(tgc.small_case(), "every"), trim=trim)


# ---- blocks, finish, reset, the order of the setters ---------------------------------------------------------------------------------

def test_one_block_two_and_seven_agree_and_the_sites_may_follow_the_references(pkg):
    c = tgc.small_case()
    sites = site_list(c, "every")
    n = len(c.recs)
    whole, kept = run(pkg, c, sites)
    check(c, whole, kept, sites)
    for cuts in ([0, n // 2, n], [round(k * n / 7) for k in range(8)]):
        got, kept_b = run(pkg, c, sites, cuts=cuts)
        check(c, got, kept_b, sites)
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], whole[:4])) and got[4] == whole[4] and bytes(kept_b) == bytes(kept)
    late, kept_l = run(pkg, c, sites, sites_after_refs=True)
    assert all(np.array_equal(x, y) for x, y in zip(late[:4], whole[:4])) and late[4] == whole[4] and bytes(kept_l) == bytes(kept)


def test_finish_twice_more_blocks_after_a_finish_and_reset(pkg):
    c = tgc.small_case()
    sites = site_list(c, "duplicates_unsorted") + site_list(c, "margins")
    n = len(c.recs)
    (a, oa), (b, ob) = blocks_of(pkg, c.raw, [0, n // 3, n])
    eng = c.engine(pkg)
    try:
        send(eng, sites, 1)
        eng.set_record_sink()
        c.genome(eng)
        empty = eng.finish_sites()
        assert not empty[3].any() and empty[4]["covered"] == empty[4]["bases"] == 0 and empty[4]["resolved"] == empty[0].size > 0
        eng.submit(a, oa)
        first, again = eng.finish_sites(), eng.finish_sites()
        kept_a = eng.finish_records()
        check(c, first, kept_a, sites, trim=1)
        assert all(np.array_equal(x, y) for x, y in zip(first[:4], again[:4])) and first[4] == again[4]
        eng.submit(b, ob)
        both = eng.finish_sites()
        whole = np.concatenate([kept_a, eng.finish_records()])
        check(c, both, whole, sites, trim=1)                                              # everything since create
        assert both[4]["bases"] > first[4]["bases"] > 0
        eng.reset()
        zero = eng.finish_sites()
        assert not zero[3].any() and np.array_equal(zero[0], both[0]) and np.array_equal(zero[1], both[1]) and np.array_equal(zero[2], both[2])
        eng.submit(c.raw)                                                                 # the sites and the trim survived the reset
        check(c, eng.finish_sites(), whole, sites, trim=1)
        assert bytes(eng.finish_records()) == bytes(whole)
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            send(eng, sites)                                                              # records have been tallied
    finally:
        eng.close()


def test_a_reference_list_that_grows_between_blocks_keeps_the_counts_and_a_new_genome_starts_from_zero(pkg):
    """SAM text: the list grows as new RNAMEs show up, and the table is packed again while blocks have been counted"""
    c = tgc.small_case()
    sites = site_list(c, "every")
    names = [n for n, _ in c.refs]
    early = [r for r in c.recs if r.rname in names[:3]]
    late = [r for r in c.recs if r.rname not in names[:3]]
    assert early and late
    eng = c.engine(pkg)
    try:
        send(eng, sites)
        eng.set_record_sink()
        eng.set_genome_arrays(c.loaded())
        eng.set_references(names[:3])
        eng.submit(tl.raw_records(c.refs, early))
        first = eng.finish_sites()
        assert set(int(r) for r in first[0]) == {0, 2} and first[4]["bases"] > 0           # (the second of the three is the ghost)
        eng.set_references(names)
        eng.submit(tl.raw_records(c.refs, late))
        got = eng.finish_sites()
        kept = eng.finish_records()
        _, want = check(c, got, kept, sites)
        assert got[4]["bases"] > first[4]["bases"] and np.array_equal(got[3][got[0] == 0], first[3][first[0] == 0])
        c.genome(eng)                                                                     # the same genome once more
        assert not eng.finish_sites()[3].any()
        eng.submit(c.raw)
        again = eng.finish_sites()
        check(c, again, eng.finish_records(), sites)
    finally:
        eng.close()


# ---- every filter in front of it, and the coverage beside it -------------------------------------------------------------------------

@pytest.mark.parametrize("combo", ["-d", "-T", "-y", "-n", "-R", "-Q"])
def test_with_every_filter_the_counts_are_those_of_the_sinks_records(pkg, combo):
    c = tgc.fuzz_case(with_rg=True, read_group="grpA") if combo == "-R" else tgc.fuzz_case()
    kw = dict(tgc.COMBOS[combo])
    if kw.pop("regions", False):
        kw["before"] = lambda eng: tgc._regions(eng, c)
    if "read_score" in kw:
        W = np.zeros((4, 8, 8), dtype=np.int16)
        W[1] = 100
        kw["read_score"] = dict(weights=W, min_score=50)
    sites = [(n, p) for n, ln in c.lens.items() for p in range(0, ln, 3)]
    got, kept = run(pkg, c, sites, trim=1, **kw)
    _, want = check(c, got, kept, sites, trim=1, min_bq=25 if combo == "-Q" else 0)
    assert 0 < len(dl.split_raw(kept)) < len(c.recs) and int(want.sum()) > 0


def test_beside_coverage_the_ten_counters_sum_to_the_devices_own_depth(pkg):
    c = tgc.small_case()
    sites = site_list(c, "every")
    eng = c.engine(pkg)
    try:
        eng.set_coverage(True)
        send(eng, sites)
        eng.set_record_sink()
        c.genome(eng)
        eng.submit(c.raw)
        got = eng.finish_sites()
        rref, rst, ren, rdp = eng.finish_coverage_runs()
        check(c, got, eng.finish_records(), sites)
    finally:
        eng.close()
    depth = {i: np.zeros(ln, dtype=np.int64) for i, (n, ln) in enumerate(c.refs) if n in c.lens}
    for r, a, b, d in zip(rref, rst, ren, rdp):
        depth[int(r)][int(a):int(b)] = int(d)
    want = np.array([depth[int(r)][int(p)] for r, p in zip(got[0], got[1])])
    assert np.array_equal(got[3].astype(np.int64).sum(axis=1), want) and int(want.max()) >= 300


# ---- the setting off: what the engine launched and allocated before ------------------------------------------------------------------

def test_setting_off_launches_and_counts_what_the_parent_commit_did(pkg):
    contigs, refs, recs = tl.fuzz_dataset(*tgc.OFF_INPUT)
    held = {n: len(q) for n, q in contigs}
    name = next(n for n, _ in refs if held.get(n, 0) > 200)
    for mode in ("off", "none", "toggled", "on"):
        eng = pkg.Engine(pss=dict(region_len=15))
        try:
            if mode == "none":
                eng.set_sites([], [], [])                    # n_sites == 0
            if mode in ("toggled", "on"):
                eng.set_sites([name], [0, 0], [100, 200])
            if mode == "toggled":                            # on and off again is off
                eng.set_sites([name], [], [])
            eng.set_genome_arrays(tl.loaded_contigs(contigs))
            eng.set_references([n for n, _ in refs])
            eng.kernel_time()
            eng.submit(tl.raw_records(refs, recs))
            eng.sync()
            assert eng.kernel_time()[1] == tgc.OFF_LAUNCHES  # (on: the time and the launch count stay the tally's)
            assert eng.counters_device()[1] == tgc.OFF_N_U64
            if mode == "on":
                assert eng.finish_sites()[0].size == 2
            else:
                with pytest.raises(pkg.PssbamError, match=EINVAL):
                    eng.finish_sites()
        finally:
            eng.close()


# ---- the calls' own rules ------------------------------------------------------------------------------------------------------------

def test_refusals(pkg):
    kmer = pkg.Engine(kmer=dict(klen=4))
    try:
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            kmer.set_sites(["c"], [0], [5])                  # not without the substitution tally
        kmer.set_sites(["c"], [], [])                        # switching off what is off is always legal
    finally:
        kmer.close()
    eng = pkg.Engine(pss=dict(region_len=5))
    try:
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_sites()                               # the setting is off
        eng.set_gapped(True)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_sites(["c"], [0], [5])
        eng.set_gapped(False)
        eng.set_sites(["c"], [0], [5])
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_gapped(True)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_sites(["c"], [0], [5], trim=65536)
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.set_sites(["c"], [1], [5])                   # a contig index outside the names
        got = eng.finish_sites()                             # no references yet: nothing is resolved
        assert got[0].size == 0 and got[4] == {"given": 1, "resolved": 0, "covered": 0, "bases": 0}
        eng.set_sites(["c"], [], [])
        eng.set_gapped(True)                                 # off again, the two go in this order too
    finally:
        eng.close()
    c = tgc.small_case()
    sites = site_list(c, "margins")
    eng = c.engine(pkg)
    try:
        send(eng, sites)
        eng.set_record_sink()
        c.genome(eng)
        eng.submit(c.raw)
        n = eng.finish_sites()[0].size
        assert n > 4
        with pytest.raises(pkg.PssbamError, match=EINVAL):
            eng.finish_sites(cap=n - 1)                      # too little room
        more = eng.finish_sites(cap=n + 5)                   # more than needed is fine
        check(c, more, eng.finish_records(), sites)
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            send(eng, sites)                                 # after the first submit
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.set_sites([], [], [])
    finally:
        eng.close()

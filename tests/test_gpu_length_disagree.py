"""Every tally arm on reads whose SEQ, CIGAR and TLEN disagree, against the oracle.

Two thirds of the 3 200 records of each dataset are proper pairs whose CIGAR is `<|TLEN|>M` while SEQ holds fewer bases
(down to one, or none: SEQ *), as many, or more (up to twice as many): length_disagree_lib.  The kernels carry code for
exactly this case -- read_nibble returns 0 past l_seq, the staged arms blank the codes at or past l_seq (and their
qualities under -Q), count_mismatches stops at min(L, l_seq), the interior walk of -W stops at min(L - d, l_seq), the
3' window sits at SEQ[L-1-i] -- and no other test runs it beyond first mates with a shorter SEQ under -n / -N and -W.
Their QUAL bytes are made of base codes, so a kernel that reads past SEQ changes a cell.

The engine always gets the records as they are.  Every pss expectation is the arm's own feature expectation, built on
the CPU from normalise(recs) (SEQ cut to |TLEN| bases or N-padded up to them) the way the arm's feature test builds it;
the k-mer expectation is the oracle's on the records as they are (fragkon filters a disagreeing record).
test_length_disagree_host.py shows without a GPU that the oracle itself obeys that rule on these very records, that three
wrong kernels would be caught, and that normalise commutes with each feature lib.  Launch shapes, Arm and run_arm (and
through it check) are test_gpu_tile_loop's.  Bit-exact (integer work)."""
import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import composition_lib as cl
import end_condition_lib as ec
import gapped_lib as gl
import interior_lib as il
import length_disagree_lib as ld
import mismatch_lib as ml
import pssbam_testlib as tl
import regions_lib as rl
import replicates_lib as rp
import site_context_lib as sc
from test_gpu_contig_sets import oracle_sets
from test_gpu_length_bins import bins_of, oracle_bins
from test_gpu_length_hist import CLASSES, flag_class, oracle_ok_rows
from test_gpu_per_contig import oracle_planes
from test_gpu_read_groups import first_rg
from test_gpu_tile_loop import (CONTIG_SETS, END_COND, HIST_MAX, LEN_EDGES, RG_IDS, SHAPES, Arm, Data, direct_hist,
                                region_stats, run_arm, sam_of, set_env, stats_of)

pytestmark = pytest.mark.gpu

SEED, N_READS, REGION = ld.SEED, ld.N_READS, ld.REGION
MISM = (10, 3)          # -N 10 -n 3
REPLICATES = 5
INTERIOR_MARGIN = 5     # -W 5
COMPOSITION = 10        # -P 10


# ---- expectations (CPU only) ------------------------------------------------------------------------------------------

def mism_hist(oracle, g, tmp, refs, contigs, recs, o: tl.PssOpts, m_max: int, k: int, tv: bool):
    """(mf, mr) of -N m_max -n k: the reads of recs added to the forward / reverse table by their mismatch bin, rows
    above k zero.  Counted with site_context_lib's direct count, and checked class by class against the oracle's PSS_OK
    on every (flag class, bin) subset."""
    ctg = dict(contigs)
    by_class = {c: (np.zeros(m_max + 2, dtype=np.uint64), np.zeros(m_max + 2, dtype=np.uint64)) for c in CLASSES}
    subsets = {}
    for r in recs:
        m = ml.mismatches(r, ctg, tv)
        if m is None:
            continue
        b = min(m, m_max + 1)
        f, rv = sc.direct_counts(contigs, [r], o, None)
        by_class[flag_class(r)][0][b] += int(f.any())
        by_class[flag_class(r)][1][b] += int(rv.any())
        subsets.setdefault((flag_class(r), b), []).append(r)
    zero = np.zeros(m_max + 2, dtype=np.uint64)
    for c in CLASSES:
        rows = zero.copy()
        for b in range(m_max + 2):
            if (c, b) in subsets:
                rows[b] = oracle.pss(g, sam_of(tmp, "mism_bin.sam", refs, subsets[(c, b)]), o)[2][tl.ST_OK]
        hf, hr = by_class[c]
        want = {"unpaired": (rows, rows), "first": (rows, zero), "second": (zero, rows)}.get(c)
        assert (np.array_equal(hf, want[0]) and np.array_equal(hr, want[1])) if want else np.array_equal(hf + hr, rows), c
    mf, mr = sum(v[0] for v in by_class.values()), sum(v[1] for v in by_class.values())
    assert mf[:k + 1].all() and mr[:k + 1].all() and mf[k + 1:].any() and mr[k + 1:].any() and not np.array_equal(mf, mr)
    mf[k + 1:] = 0
    mr[k + 1:] = 0
    return mf, mr


def build_arms(oracle, tmp):
    """-> (datasets, arms).  Nothing here touches a GPU."""
    D, A = {}, {}
    D["main"] = Data(*ld.dataset(SEED, N_READS, REGION))
    D["sets"] = Data(*ld.dataset(SEED + 1, N_READS, REGION, contig_lens=(5000, 1200, 300, 900)))
    D["rg"] = Data(*ld.dataset(SEED + 2, N_READS, REGION, with_rg=True))
    c, f, r = ld.dataset(SEED + 3, N_READS, REGION)
    own = {id(x) for x in ld.crafted(r)}
    dmg = iter(ec.plant_damage(c, [x for x in r if id(x) not in own], np.random.default_rng(SEED + 4), 0.5))
    D["dmg"] = Data(c, f, [x if id(x) in own else next(dmg) for x in r])       # damage on the ordinary (unpaired) third only
    for d in D.values():
        odd = [x for x in ld.crafted(d.recs) if ld.kind(x) != "equal"]
        assert len(d.recs) == N_READS and len(odd) > 1800 and {ld.kind(x) for x in odd} == {"short", "long", "star"}

    def table_pair(t):
        assert t[0][2:].any() and t[1][2:].any() and t[0][:2].any() and t[1][:2].any()
        return t[0], t[1]

    # ---- the main dataset ---------------------------------------------------------------------------------------------
    p = D["main"]
    norm = ld.normalise(p.recs)
    g = oracle.genome_from_arrays(p.loaded)
    as_is, sam = sam_of(tmp, "as_is.sam", p.refs, p.recs), sam_of(tmp, "norm.sam", p.refs, norm)
    kmer, kst = {}, {}
    for k in (4, 5):
        k5, k3, kst[k] = oracle.fragkon(g, as_is, tl.FkOpts(klen=k))
        assert k5.any() and k3.any()
        kmer[k] = (k5, k3)
    plain = {}
    for n in (7, 15, 16, 25, 40):
        wf, wr, st = oracle.pss(g, sam, tl.PssOpts(region_len=n))
        assert st[tl.ST_OK] > 0.6 * N_READS        # (two thirds of the records disagree: most of what is tallied does)
        plain[n] = (table_pair((wf, wr)), st)

    def plain_arm(n, k=None, **more):
        return Arm("main", dict(pss=dict(region_len=n), kmer=dict(klen=k) if k else None),
                   dict(tables=plain[n][0], kmer=kmer[k] if k else None, stats=stats_of(N_READS, plain[n][1], kst[k] if k else None)), **more)

    # tally_compact (-r <= 16) and, under KERNEL_SIMPLE, tally_simple; tally_tiled above (-r 40: the second row pass)
    A["compact_r7"], A["compact_r16"], A["compact_r16_k4"] = plain_arm(7), plain_arm(16), plain_arm(16, 4)
    A["plan_once_r15"] = plain_arm(15, env={"PSSBAM_COMPACT_PLAN_ONCE": "1"})
    A["tiled_r25"], A["tiled_r40"], A["tiled_r25_k5"] = plain_arm(25), plain_arm(40), plain_arm(25, 5)
    # -Q 20: the qualities at or past l_seq are blanked with the codes
    masked = sam_of(tmp, "q20.sam", p.refs, bq.mask_recs(norm, 20))
    for n in (25, 40):
        wf, wr, st = oracle.pss(g, masked, tl.PssOpts(region_len=n))
        assert (wf[2:] != plain[n][0][0][2:]).any() and (wr[2:] != plain[n][0][1][2:]).any()
        A[f"Q20_r{n}"] = Arm("main", dict(pss=dict(region_len=n), min_base_qual=20), dict(tables=table_pair((wf, wr)), stats=stats_of(N_READS, st)))
    # -T
    ivs = rl.fuzz_intervals(SEED, p.contigs, p.recs)
    red = sam_of(tmp, "red.sam", p.refs, rl.reduce_recs(norm, ivs))
    for n in (15, 40):
        wf, wr, st = oracle.pss(g, red, tl.PssOpts(region_len=n))
        assert 0 < st[tl.ST_OK] < plain[n][1][tl.ST_OK]
        A[f"T_r{n}"] = Arm("main", dict(pss=dict(region_len=n)), dict(tables=table_pair((wf, wr)), stats=region_stats(N_READS, plain[n][1], st)), regions=ivs)
    # -H 100: a paired read's row is |TLEN|, whatever SEQ holds
    o = tl.PssOpts(region_len=25)
    by_class = direct_hist(p.contigs, norm, o, HIST_MAX)
    zero = np.zeros(HIST_MAX + 2, dtype=np.uint64)
    for c in CLASSES:
        rows = oracle_ok_rows(oracle, g, sam_of(tmp, f"h_{c}.sam", p.refs, [x for x in norm if flag_class(x) == c]), o, HIST_MAX)
        hf, hr = by_class[c]
        want = {"unpaired": (rows, rows), "first": (rows, zero), "second": (zero, rows)}.get(c)
        assert (np.array_equal(hf, want[0]) and np.array_equal(hr, want[1])) if want else np.array_equal(hf + hr, rows), c
    hf, hr = sum(v[0] for v in by_class.values()), sum(v[1] for v in by_class.values())
    assert hf[40:101].sum() > 500 and hr[40:101].sum() > 500 and hf[101] > 0 and hr[101] > 0 and not np.array_equal(hf, hr)
    A["H100_r25"] = Arm("main", dict(pss=dict(region_len=25), length_hist=HIST_MAX), dict(tables=plain[25][0], hist=(hf, hr), stats=stats_of(N_READS, plain[25][1])))
    # -X cpg
    w_in, w_out = (table_pair(oracle.pss(g, sam_of(tmp, f"site{int(keep)}.sam", p.refs, sc.mask_recs(p.contigs, norm, keep)), o)[:2]) for keep in (True, False))
    A["X_r25"] = Arm("main", dict(pss=dict(region_len=25), site_context="cpg"), dict(tables=plain[25][0], site=(w_in, w_out), stats=stats_of(N_READS, plain[25][1])))
    # -I: a <T>M record whose SEQ is not T bases long does not anchor and falls under the plain rule, in the GAPPED arm
    wf, wr, st = oracle.pss(g, sam_of(tmp, "anchored.sam", p.refs, gl.anchor_recs(norm)), o)
    assert st[tl.ST_OK] > plain[25][1][tl.ST_OK]
    A["I_r25"] = Arm("main", dict(pss=dict(region_len=25), gapped=True), dict(tables=table_pair((wf, wr)), stats=stats_of(N_READS, st)))
    # -n 3 -N 10, and with -V
    for tv in (False, True):
        wf, wr, st = oracle.pss(g, sam_of(tmp, "mism.sam", p.refs, ml.reduce_to(norm, p.contigs, MISM[1], tv)), o)
        assert 0 < st[tl.ST_OK] < plain[25][1][tl.ST_OK]
        stats = stats_of(N_READS, plain[25][1])
        stats.update(pss_ok=int(st[tl.ST_OK]), pss_filtered=int(plain[25][1][tl.ST_FILTERED] + plain[25][1][tl.ST_OK] - st[tl.ST_OK]))
        A["mism_r25" + ("_V" if tv else "")] = Arm("main", dict(pss=dict(region_len=25), mismatches=(*MISM, int(tv))), dict(
            tables=table_pair((wf, wr)), stats=stats, mism=mism_hist(oracle, g, tmp, p.refs, p.contigs, norm, o, *MISM, tv)))
    # -S: planes by |TLEN|
    for n in (25, 40):
        on = tl.PssOpts(region_len=n)
        bins = {key: table_pair(t) for key, t in oracle_bins(oracle, g, sam, on, LEN_EDGES[n]).items()}
        assert list(bins) == bins_of(on, LEN_EDGES[n])
        A[f"S_r{n}"] = Arm("main", dict(pss=dict(region_len=n), length_bins=LEN_EDGES[n]), dict(tables=plain[n][0], planes=("bins", bins), stats=stats_of(N_READS, plain[n][1])))
    # -J 5: read-name replicates
    reps = [table_pair(oracle.pss(g, sam_of(tmp, "rep.sam", p.refs, rp.reduce(norm, REPLICATES, j)), o)[:2]) for j in range(REPLICATES)]
    A["J5_r25"] = Arm("main", dict(pss=dict(region_len=25), replicates=REPLICATES), dict(tables=plain[25][0], replicates=reps, stats=stats_of(N_READS, plain[25][1])))
    # -W 5 (and under -Q 20) and -P 10: the interior is { i : d <= i, i + d < L, i < l_seq }, so the table is that of the
    # normalised records (cut at L, N beyond l_seq); `reads` counts the records whose interior is not empty, which a
    # record with l_seq <= d is not: that count comes from the records as they are.  -P looks at the reference alone.
    ctg = dict(p.contigs)
    entered = {k: [x for x in ld.crafted(p.recs) if ld.kind(x) == k and any(il.tables_entered(x, ctg, o))] for k in ("short", "long", "star")}
    assert min(len(v) for v in entered.values()) >= 50, {k: len(v) for k, v in entered.items()}     # each kind is among the reads added to a table
    for q in (0, 20):
        table, n_norm, tallied = il.interior(norm, p.contigs, INTERIOR_MARGIN, o, q)
        as_is_table, reads, as_is_tallied = il.interior(p.recs, p.contigs, INTERIOR_MARGIN, o, q)
        assert np.array_equal(table, as_is_table) and tallied == as_is_tallied == plain[25][1][tl.ST_OK] and table.all()
        empty = sum(1 for x in p.recs if ld.governed(x) and any(il.tables_entered(x, ctg, o))
                    and (0 if x.seq == "*" else len(x.seq)) <= INTERIOR_MARGIN < abs(x.tlen) - INTERIOR_MARGIN)
        assert 0 < empty == n_norm - reads                                      # SEQ ends before the interior begins
        for k in ("short", "long"):     # ... and each of these kinds adds bases of its own (a star read has none)
            assert il.interior(entered[k], p.contigs, INTERIOR_MARGIN, o, q)[0].any(), k
        tabs = plain[25][0] if not q else A["Q20_r25"].want["tables"]
        A["W5_r25" if not q else "W5_Q20_r25"] = Arm("main", dict(pss=dict(region_len=25), interior=INTERIOR_MARGIN, min_base_qual=q),
                                                     dict(tables=tabs, interior=(table, reads), stats=stats_of(N_READS, plain[25][1])))
    assert int(A["W5_Q20_r25"].want["interior"][0].sum()) < int(A["W5_r25"].want["interior"][0].sum())
    c5, c3, n_fwd, n_rev = cl.composition(norm, p.contigs, COMPOSITION, o)
    assert all(np.array_equal(a, b) for a, b in zip((c5, c3), cl.composition(p.recs, p.contigs, COMPOSITION, o)[:2])) and n_fwd > 500 and n_rev > 500
    for k, sub in entered.items():
        k5, k3, _, _ = cl.composition(sub, p.contigs, COMPOSITION, o)
        assert k5.any() and k3.any(), k
    A["P10_r25"] = Arm("main", dict(pss=dict(region_len=25), composition=COMPOSITION), dict(tables=plain[25][0], composition=(c5, c3), stats=stats_of(N_READS, plain[25][1])))
    oracle.free_genome(g)

    # ---- -C and -A: four contigs ----------------------------------------------------------------------------------------
    s = D["sets"]
    g = oracle.genome_from_arrays(s.loaded)
    sam = sam_of(tmp, "sets.sam", s.refs, ld.normalise(s.recs))
    wf, wr, st = oracle.pss(g, sam, o)
    sets = {key: table_pair(t) for key, t in oracle_sets(oracle, s.contigs, sam, o, CONTIG_SETS).items()}
    assert (wf - sum(t[0] for t in sets.values()))[2:].any()
    A["C_r25"] = Arm("sets", dict(pss=dict(region_len=25), contig_sets=CONTIG_SETS), dict(tables=table_pair((wf, wr)), planes=("sets", sets), stats=stats_of(N_READS, st)))
    planes = oracle_planes(oracle, s.contigs, s.refs, sam, o)
    assert len(planes) == 4
    A["A_r25"] = Arm("sets", dict(pss=dict(region_len=25), per_contig=True), dict(tables=(wf, wr), contigs=planes, stats=stats_of(N_READS, st)))
    oracle.free_genome(g)

    # ---- -G: two IDs and the unassigned bucket ----------------------------------------------------------------------------
    q = D["rg"]
    g = oracle.genome_from_arrays(q.loaded)
    norm = ld.normalise(q.recs)
    wf, wr, st = oracle.pss(g, sam_of(tmp, "rg.sam", q.refs, norm), o)
    groups = {}
    for key in [None] + RG_IDS:
        sel = [x for x in norm if (first_rg(x) == key if key is not None else first_rg(x) not in RG_IDS)]
        groups[key] = table_pair(oracle.pss(g, sam_of(tmp, "grp.sam", q.refs, sel), o)[:2])
    A["G_r25"] = Arm("rg", dict(pss=dict(region_len=25), read_groups=RG_IDS), dict(tables=table_pair((wf, wr)), planes=("groups", groups), stats=stats_of(N_READS, st)))
    oracle.free_genome(g)

    # ---- -E ds,2: a paired read is neither marked nor added to a COND table -------------------------------------------------
    d = D["dmg"]
    g = oracle.genome_from_arrays(d.loaded)
    norm = ld.normalise(d.recs)
    wf, wr, st = oracle.pss(g, sam_of(tmp, "dmg.sam", d.refs, norm), o)
    cf, cr, reads = ec.expected(oracle, g, tmp, d.refs, d.contigs, norm, o, *END_COND)
    assert cf[2:].any() and cr[2:].any() and reads[0] > reads[1] >= 20 and reads[0] > reads[2] >= 20 and reads[3] >= 5
    ordinary = [x for x in norm if not x.qname.startswith("d")]
    assert all(np.array_equal(a, b) for a, b in zip((cf, cr, reads), ec.expected(oracle, g, tmp, d.refs, d.contigs, ordinary, o, *END_COND)))
    A["E_ds2_r25"] = Arm("dmg", dict(pss=dict(region_len=25), end_condition=END_COND), dict(tables=table_pair((wf, wr)), end=(cf, cr, reads), stats=stats_of(N_READS, st)))
    oracle.free_genome(g)
    return D, A


# ---- the cases ------------------------------------------------------------------------------------------------------

COMPACT = ["compact_r7", "compact_r16", "compact_r16_k4", "plan_once_r15"]
TILED = ["tiled_r25", "tiled_r40", "tiled_r25_k5", "Q20_r25", "Q20_r40", "T_r15", "T_r40", "H100_r25", "X_r25", "I_r25", "mism_r25", "mism_r25_V", "E_ds2_r25",
         "W5_r25", "W5_Q20_r25", "P10_r25"]
PLANES = ["S_r25", "S_r40", "C_r25", "G_r25", "A_r25", "J5_r25"]
OVERFLOW = ["tiled_r25", "Q20_r25", "I_r25", "W5_r25", "W5_Q20_r25", "P10_r25"]
SIMPLE = ["compact_r7", "tiled_r40", "tiled_r25_k5", "Q20_r25", "T_r15", "H100_r25", "X_r25", "I_r25", "mism_r25", "mism_r25_V", "E_ds2_r25",
          "S_r25", "C_r25", "G_r25", "A_r25", "J5_r25", "W5_r25", "W5_Q20_r25", "P10_r25"]
FEED = ["plan_once_r15", "Q20_r25"]      # (plain -r 15; the environment of plan_once is not set for the feed)


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


@pytest.fixture(scope="module")
def built(oracle, tmp_path_factory):
    D, A = build_arms(oracle, tmp_path_factory.mktemp("length_disagree_gpu"))
    assert set(COMPACT + TILED + PLANES + OVERFLOW + SIMPLE + FEED) <= set(A)
    return D, A


def case(pkg, built, monkeypatch, name, shape=None, kernel=None, feed=None, env=True):
    arm = built[1][name]
    set_env(monkeypatch, SHAPES[shape] if shape else {}, arm.env if env else {})
    tot, _ = run_arm(pkg, built, name, pkg.KERNEL_AUTO if kernel is None else kernel, feed=feed)
    return tot


@pytest.mark.parametrize("shape", [None, "three_wg"], ids=["default_grid", "three_wg"])
@pytest.mark.parametrize("name", COMPACT + TILED + PLANES)
def test_arms(pkg, built, monkeypatch, name, shape):
    """tally_compact, tally_tiled with each option arm, and the plane kernels: one tile per workgroup, and several"""
    case(pkg, built, monkeypatch, name, shape)


@pytest.mark.parametrize("name", OVERFLOW)
def test_one_lane_path(pkg, built, monkeypatch, name):
    """five staged pieces: the records past the staged prefix are tallied by one lane from global memory"""
    tot = case(pkg, built, monkeypatch, name, "two_wg_overflow")
    assert tot.stats["slow_path"] > 0


@pytest.mark.parametrize("name", SIMPLE)
def test_lane_per_read_kernels(pkg, built, monkeypatch, name):
    """tally_simple and its plane form (read_nibble, count_mismatches)"""
    case(pkg, built, monkeypatch, name, kernel=pkg.KERNEL_SIMPLE, env=False)


@pytest.fixture(scope="module")
def bam_feed(built, tmp_path_factory):
    """the main dataset as a BGZF BAM in 300-byte blocks"""
    d = built[0]["main"]
    bam = tmp_path_factory.mktemp("length_disagree_feed") / "x.bam"
    tl.write_bam(bam, d.refs, d.recs, block=300)
    return np.frombuffer(bam.read_bytes(), dtype=np.uint8), len(tl.bam_bytes(d.refs, []))


@pytest.mark.parametrize("name", FEED)
def test_compressed_feed(pkg, built, bam_feed, monkeypatch, name):
    """inflated and indexed on the device; run_arm asserts that the feed flags are 0"""
    case(pkg, built, monkeypatch, name, feed=bam_feed, env=False)

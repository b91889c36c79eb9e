"""No GPU: the yardstick of test_gpu_length_disagree.py on the CPU oracle.

A paired `<|TLEN|>M` record is tallied as if SEQ were cut to |TLEN| bases or N-padded on the right up to |TLEN| bases
(length_disagree_lib.normalise).  Here the oracle shows that on the very dataset the GPU test feeds the engine, that
most of the disagreeing records are tallied, that the dataset covers every residue of l_seq mod 8 and every record
offset mod 16, that three wrong models (the 3' end anchored on l_seq; missing bases read from QUAL; the interior walk
of -W running to L - d whatever l_seq) give other tables, and that normalise commutes with every feature lib the GPU test builds its expectations with.  Bit-exact."""
from collections import Counter

import numpy as np
import pytest

import base_quality_lib as bq
import composition_lib as cl
import gapped_lib as gl
import interior_lib as il
import length_disagree_lib as ld
import mismatch_lib as ml
import pssbam_testlib as tl
import regions_lib as rl
import site_context_lib as sc
from test_gpu_contig_sets import oracle_sets
from test_gpu_length_bins import oracle_bins
from test_gpu_tile_loop import CONTIG_SETS, HIST_MAX, LEN_EDGES, direct_hist

SEED, N_READS, REGION = ld.SEED, ld.N_READS, ld.REGION      # the GPU test's main dataset
ROWS = (7, 16, 25, 40)


@pytest.fixture(scope="module")
def case(oracle, tmp_path_factory):
    contigs, refs, recs = ld.dataset(SEED, N_READS, REGION)
    tmp = tmp_path_factory.mktemp("length_disagree")
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))

    def run(name, rs, n, **kw):
        tl.write_sam(tmp / name, refs, rs)
        return oracle.pss(g, tmp / name, tl.PssOpts(region_len=n, **kw))

    yield dict(contigs=contigs, refs=refs, recs=recs, norm=ld.normalise(recs), run=run, g=g, tmp=tmp)
    oracle.free_genome(g)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_record_mix(case):
    recs = case["recs"]
    own = ld.crafted(recs)
    assert len(recs) == N_READS and 0.6 * N_READS < len(own) < 0.73 * N_READS
    kinds = Counter(ld.kind(r) for r in own)
    assert min(kinds[k] for k in ("short", "equal", "long", "star")) >= 80 and kinds["short"] > 700 and kinds["long"] > 700
    assert all(ld.governed(r) and (r.flag & 0xB) == 0x3 and REGION <= abs(r.tlen) <= REGION + 80 for r in own)
    assert all(set(ord(c) - 33 for c in r.qual) <= set(ld.QUAL_VALUES) for r in own if r.qual != "*")
    lens = dict(case["refs"])
    assert all(2 <= r.pos - 1 <= lens[r.rname] - abs(r.tlen) - 2 for r in own)
    for mate, strand in ld.CLASSES:
        share = sum((r.flag & 0xD0) == mate | strand for r in own) / len(own)
        assert 0.22 < share < 0.28
    assert 0.45 < sum(r.tlen > 0 for r in own) / len(own) < 0.55
    # every SEQ length the issue names occurs, relative to some N of the row passes
    for r_len in (7, 16, 25, 40):
        rel = {(len(r.seq) - r_len, len(r.seq) - abs(r.tlen) + r_len) for r in own if r.seq != "*"}
        assert {-1, 0, 1} <= {a for a, _ in rel} and {-1, 0, 1} <= {b for _, b in rel}, r_len
    assert {1, 2} <= {len(r.seq) for r in own} and {-1, 1, 2} <= {len(r.seq) - abs(r.tlen) for r in own}
    assert any(len(r.seq) == 2 * abs(r.tlen) for r in own) and max(len(r.seq) - abs(r.tlen) for r in own) > 150


def test_residues_and_offsets(case):
    """among the TALLIED disagreeing reads of each mate-by-strand class every l_seq mod 8 (hence both parities) occurs
    20 times or more, at -r 40 where the fewest are tallied; records start at every offset mod 16"""
    o = tl.PssOpts(region_len=REGION)
    seen = {c: Counter() for c in ld.CLASSES}
    offs = set()
    for r, off in zip(case["recs"], ld.record_offsets(case["refs"], case["recs"])):
        if r.qname.startswith("d") and ld.kind(r) != "equal":
            f, rv = sc.direct_counts(case["contigs"], [r], o, None)
            if f.any() or rv.any():
                seen[(r.flag & 0xC0, r.flag & 0x10)][(0 if r.seq == "*" else len(r.seq)) % 8] += 1
                offs.add(off % 16)
    for c, cnt in seen.items():
        assert sorted(cnt) == list(range(8)) and min(cnt.values()) >= 20, (c, dict(cnt))
    assert offs == set(range(16))
    assert {len(r.qname) for r in ld.crafted(case["recs"])} == set(range(1, 41))


@pytest.mark.parametrize("n", ROWS)
def test_oracle_equivalence(case, n):
    """tables and status counters of the records as they are == those of the normalised records"""
    a = case["run"]("asis.sam", case["recs"], n)
    b = case["run"]("norm.sam", case["norm"], n)
    assert same(a, b)
    assert a[0][2:].any() and a[1][2:].any() and all(a[2][s] > 0 for s in (tl.ST_OK, tl.ST_PARSE_SKIP, tl.ST_NO_CONTIG, tl.ST_FILTERED))


@pytest.mark.parametrize("n", ROWS)
def test_share_tallied(case, n):
    """the floor is 60 % of the disagreeing records; this seed tallies more than 95 % of them at every -r"""
    odd = [r for r in ld.crafted(case["recs"]) if ld.kind(r) != "equal"]
    st = case["run"]("odd.sam", odd, n)[2]
    assert len(odd) > 1800 and st[tl.ST_OK] >= 0.6 * len(odd) and st[tl.ST_OK] >= 0.95 * len(odd), (int(st[tl.ST_OK]), len(odd))


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("which", ["short", "long"])
def test_wrong_models_give_other_tables(case, which, n):
    """the 3' end anchored on l_seq: other tables for short and for long SEQ.  Missing bases read from the QUAL nibbles:
    other tables for short SEQ; a long SEQ has no missing base, and there the model must be the identity.  The -W walk
    that runs to L - d and ignores l_seq reads those same nibbles: another interior table for short SEQ, with and without
    -Q 20 (the bytes behind a short SEQ are QUAL, so the wrong walk also takes its qualities from the wrong place)."""
    sub = [r for r in ld.crafted(case["recs"]) if ld.kind(r) == which]
    true = case["run"]("true.sam", sub, n)
    anch = case["run"]("anchor.sam", ld.anchor_on_l_seq(sub), n)
    assert (anch[0][2:] != true[0][2:]).any() and (anch[1][2:] != true[1][2:]).any()
    assert np.array_equal(anch[2], true[2])
    assert np.array_equal(anch[0][:2], true[0][:2]) and np.array_equal(anch[1][:2], true[1][:2])     # context rows do not look at SEQ
    if which == "short":
        unb = case["run"]("unblanked.sam", ld.unblanked(sub), n)
        assert (unb[0][2:] != true[0][2:]).any() and (unb[1][2:] != true[1][2:]).any()
        masked = case["run"]("unblanked_q20.sam", bq.mask_recs(ld.unblanked(sub), 20), n)           # and with -Q 20 still
        true_q = case["run"]("true_q20.sam", bq.mask_recs(ld.normalise(sub), 20), n)
        assert (masked[0][2:] != true_q[0][2:]).any() and (masked[1][2:] != true_q[1][2:]).any()
        o = tl.PssOpts(region_len=n)
        for q in (0, 20):
            right = il.interior(sub, case["contigs"], 5, o, q)
            wrong = il.interior(ld.unblanked(sub), case["contigs"], 5, o, q)
            assert right[2] == wrong[2] > 300 and (wrong[0] != right[0]).any() and wrong[1] > right[1], (q, right[1:], wrong[1:])
    else:
        assert ld.unblanked(sub) == ld.normalise(sub)


def test_normalise_commutes_with_the_feature_libs(oracle, case):
    """record for record where the lib maps records to records; through the oracle where it is a set of oracle runs"""
    contigs, recs, norm = case["contigs"], case["recs"], case["norm"]
    assert norm != recs and ld.normalise(norm) == norm
    assert all(len(r.seq) == len(r.qual) == abs(r.tlen) for r in norm if ld.governed(r))
    assert bq.mask_recs(norm, 20) == ld.normalise(bq.mask_recs(recs, 20))
    assert bq.mask_recs(norm, 20) != norm
    for keep in (True, False):
        assert sc.mask_recs(contigs, norm, keep) == ld.normalise(sc.mask_recs(contigs, recs, keep))
    ivs = rl.fuzz_intervals(SEED, contigs, recs)
    assert rl.reduce_recs(norm, ivs) == ld.normalise(rl.reduce_recs(recs, ivs))
    assert gl.anchor_recs(norm) == ld.normalise(gl.anchor_recs(recs))
    odd = [r for r in ld.crafted(recs) if ld.kind(r) != "equal"]
    assert all(gl.anchor_info(r) is None for r in odd)                   # the <T>M records do not anchor as they are
    ctg = dict(contigs)
    for tv in (False, True):
        assert [ml.mismatches(r, ctg, tv) for r in recs] == [ml.mismatches(r, ctg, tv) for r in norm]
    assert ml.reduce_to(norm, contigs, 3) == ld.normalise(ml.reduce_to(recs, contigs, 3))
    assert 0 < len(ml.reduce_to(odd, contigs, 3)) < len(odd)
    o = tl.PssOpts(region_len=25)
    for q in (0, 20):       # -W: the table and the reads added to a table commute; a record whose SEQ ends at or before d has an empty interior as it is
        x, y = il.interior(recs, contigs, 5, o, q), il.interior(norm, contigs, 5, o, q)
        assert np.array_equal(x[0], y[0]) and x[0].all() and x[2] == y[2] > 0.6 * N_READS
        ended = sum(1 for r in recs if ld.governed(r) and any(il.tables_entered(r, dict(contigs), o)) and (0 if r.seq == "*" else len(r.seq)) <= 5 < abs(r.tlen) - 5)
        assert y[1] - x[1] == ended > 50
    x, y = cl.composition(recs, contigs, 10, o), cl.composition(norm, contigs, 10, o)      # -P looks at no read base
    assert all(np.array_equal(a, b) for a, b in zip(x[:2], y[:2])) and x[2:] == y[2:] and x[0].any() and x[1].any()
    a, b = direct_hist(contigs, recs, o, HIST_MAX), direct_hist(contigs, norm, o, HIST_MAX)
    assert all(same(a[c], b[c]) for c in a)
    for name, rs in (("asis.sam", recs), ("norm.sam", norm)):
        tl.write_sam(case["tmp"] / name, case["refs"], rs)
    x = oracle_bins(oracle, case["g"], case["tmp"] / "asis.sam", o, LEN_EDGES[25])
    y = oracle_bins(oracle, case["g"], case["tmp"] / "norm.sam", o, LEN_EDGES[25])
    assert list(x) == list(y) and all(same(x[k], y[k]) and x[k][0][2:].any() for k in x)


def test_oracle_sets_commute(oracle, tmp_path):
    """-C: the oracle on the genome reduced to a set's contigs, records as they are == normalised"""
    contigs, refs, recs = ld.dataset(SEED + 1, 1200, REGION, contig_lens=(5000, 1200, 300, 900))
    for name, rs in (("asis.sam", recs), ("norm.sam", ld.normalise(recs))):
        tl.write_sam(tmp_path / name, refs, rs)
    o = tl.PssOpts(region_len=25)
    x = oracle_sets(oracle, contigs, tmp_path / "asis.sam", o, CONTIG_SETS)
    y = oracle_sets(oracle, contigs, tmp_path / "norm.sam", o, CONTIG_SETS)
    assert all(same(x[k], y[k]) for k in CONTIG_SETS) and sum(bool(x[k][0][2:].any()) for k in CONTIG_SETS) == 3


def test_fragkon_filters_a_disagreeing_record(oracle, case):
    """fragkon compares strlen(SEQ) with the CIGAR: a record whose SEQ is not |TLEN| bases long is filtered there, so the
    k-mer expectation is the oracle's on the records as they are"""
    odd = [r for r in ld.crafted(case["recs"]) if ld.kind(r) != "equal"]
    even = [r for r in ld.crafted(case["recs"]) if ld.kind(r) == "equal"]
    for k in (4, 5):
        tl.write_sam(case["tmp"] / "odd.sam", case["refs"], odd)
        k5, k3, st = oracle.fragkon(case["g"], case["tmp"] / "odd.sam", tl.FkOpts(klen=k))
        assert not k5.any() and not k3.any() and st[tl.ST_FILTERED] == len(odd)
        tl.write_sam(case["tmp"] / "even.sam", case["refs"], even)
        k5, k3, st = oracle.fragkon(case["g"], case["tmp"] / "even.sam", tl.FkOpts(klen=k))
        assert k5.any() and k3.any() and st[tl.ST_OK] > 0.9 * len(even)

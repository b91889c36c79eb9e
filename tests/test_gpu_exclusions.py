"""The engine's exclusive modes, pair by pair: with mode A on, the setter of every other mode B is refused with
"<B> and <A> exclude each other" -- both named exactly -- and changes nothing; B's "off" call is accepted all the same; and once
A is off again B goes on.  No record is submitted and no kernel is launched: this is the table of engine.hip (MODES,
check_exclusive) and the size of the counter block behind it."""
import pytest

import __graft_entry__ as ge
import read_score_lib as rs

pytestmark = pytest.mark.gpu

SCORE = dict(weights=rs.tables()["pmd"], min_score=0, hist_half=4, hist_shift=8)

# name in the messages: (Engine keyword that switches it on, setter, arguments on, arguments off or None, what the engine reports)
MODES = {
    "read groups": (dict(read_groups=["a"]), "set_read_groups", (["a"],), None, lambda e: e.read_groups == ["a"]),
    "length bins": (dict(length_bins=[30]), "set_length_bins", ([30],), None, lambda e: len(e.length_bins) == 2),
    "contig sets": (dict(contig_sets={"x": ["chrA"]}), "set_contig_sets", ({"x": ["chrA"]},), None, lambda e: e.contig_sets == ["x"]),
    "replicates": (dict(replicates=4), "set_replicates", (4,), (0,), lambda e: e.replicates == 4),
    "per-contig tables": (dict(per_contig=True), "set_per_contig", (True,), (False,), lambda e: e.per_contig),
    "the length histogram": (dict(length_hist=100), "set_length_histogram", (100,), (0,), lambda e: e.length_hist == 100),
    "site context": (dict(site_context="cpg"), "set_site_context", ("cpg",), (None,), lambda e: e.site_context == "cpg"),
    "the end condition": (dict(end_condition=(1, 13, 13)), "set_end_condition", (1, 13, 13), (0,), lambda e: e.end_condition == (1, 13, 13)),
    "gapped reads": (dict(gapped=True), "set_gapped", (True,), (False,), lambda e: e.gapped),
    "the mismatch count": (dict(mismatches=(4, -1, 0)), "set_mismatches", (4, -1, 0), (0, -1, 0), lambda e: e.mismatches == (4, -1, 0)),
    "the interior table": (dict(interior=3), "set_interior", (3,), (-1,), lambda e: e.interior == 3),
    "the composition table": (dict(composition=4), "set_composition", (4,), (0,), lambda e: e.composition == 4),
    "the read score": (dict(read_score=SCORE), "set_read_score", (SCORE["weights"], 0, 4, 8), (None,), lambda e: e.read_score is not None),
}


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def block_is_as_laid_out(eng):
    assert eng.counter_layout()["n_u64"] == eng.counters_device()[1]


@pytest.mark.parametrize("a", list(MODES))
def test_every_other_mode_is_refused_by_name_and_changes_nothing(pkg, a):
    kw_a, set_a, _, off_a, a_on = MODES[a]
    for b, (_, set_b, on_b, off_b, b_on) in MODES.items():
        if b == a:
            continue
        eng = pkg.Engine(pss=dict(region_len=5), **kw_a)
        try:
            n = eng.counters_device()[1]
            assert a_on(eng) and not b_on(eng)
            block_is_as_laid_out(eng)
            with pytest.raises(pkg.PssbamError) as err:
                getattr(eng, set_b)(*on_b)
            assert f"{b} and {a} exclude each other" in str(err.value), (a, b, str(err.value))
            assert a_on(eng) and not b_on(eng) and eng.counters_device()[1] == n
            block_is_as_laid_out(eng)
            if off_b is not None:                       # leaving one's own mode off is always legal
                getattr(eng, set_b)(*off_b)
                assert a_on(eng) and not b_on(eng) and eng.counters_device()[1] == n
                block_is_as_laid_out(eng)
            if off_a is None:                           # planes of -G / -S / -C stay: B on an engine that never had them
                eng.close()
                eng = pkg.Engine(pss=dict(region_len=5))
            else:
                getattr(eng, set_a)(*off_a)
            assert not a_on(eng)
            getattr(eng, set_b)(*on_b)
            assert b_on(eng), (a, b)
            block_is_as_laid_out(eng)
        finally:
            eng.close()

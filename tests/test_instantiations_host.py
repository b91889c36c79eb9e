"""No GPU: the census of the tiled tally family (instantiation_lib) against the launch code, and the expectations
test_gpu_instantiations.py compares the kernels with.

The counts 68 / 40 / 12 / 6 come from a Python mirror of the predicate tally_tiled_exists (tally_kernels.h) and of the
with_arm / with_flags / with_planes launch sites; the tripwire holds the statements of tally_kernels.h and engine.hip the
mirror was written from against the files.
When it trips, the instantiation table has changed: update `exists`, `launched`, COUNTS and CONFIGS in instantiation_lib
so that every new instantiation has a configuration (and an expectation), then the recorded statements.

The guards make sure no comparison of the GPU module is vacuous: -Q bites, -T keeps some reads and drops some, the two
together differ from either, planes are populated, the later row pass has rows to add, every feature table is non-zero on
both strands.  "Plane 0" is the unassigned plane where the selector has one (-G: reads of no listed group; -C: contigs
of no set); -S, -J and -A assign every tallied read, their leading plane is empty by construction, and the guard asks
the first plane of the expectation instead.

Building all 85 expectations (the module fixture, no GPU) was timed at 7.4 s on one CPU core, with the five datasets of
3 200 records test_gpu_tile_loop uses; the fixture prints the figure of the run at hand."""
import time

import numpy as np
import pytest

import inspect
import re

import instantiation_lib as inl
import test_gpu_read_score
from test_gpu_tile_loop import COMPACT


@pytest.fixture(scope="module")
def built(oracle, tmp_path_factory):
    t0 = time.perf_counter()
    D, A = inl.build_arms(oracle, tmp_path_factory.mktemp("instantiations_host"))
    print(f"\ninstantiation expectations: {time.perf_counter() - t0:.1f} s for {len(A)} configurations")
    return D, A


# ---- the census ---------------------------------------------------------------------------------------------------------

def test_counts():
    fams = inl.enumerate_all()
    assert {k: len(v) for k, v in fams.items()} == inl.COUNTS == {"tally_tiled": 68, "tally_tiled_planes": 40, "tally_tiled_kmer_planes": 12, "tally_compact": 6}
    tiled = [dict(zip(inl.TILED_FLAGS, a)) for _, a in fams["tally_tiled"]]
    assert sum(not f["LATER"] for f in tiled) == 56 and sum(f["LATER"] for f in tiled) == 12
    options = lambda f: "".join(o for o, arm in inl.OPTION_ARM.items() if f["ARM"] == arm) or "-"   # noqa: E731
    split = {}
    for f in tiled:
        key = ("kmer" if not f["DO_PSS"] else "pss_kmer" if f["DO_KMER"] else "pss", bool(f["LATER"]), options(f))
        split[key] = split.get(key, 0) + 1
    assert split == {**{("pss", False, o): 4 for o in "-HXEINWP"}, **{("pss", True, o): 4 for o in "-XI"},
                     ("pss_kmer", False, "-"): 8, ("pss_kmer", False, "H"): 8, ("kmer", False, "-"): 4, ("pss", False, "Y"): 4}
    assert all(len(set(v)) == len(v) for v in fams.values())


def test_tripwire_engine_source_is_what_the_census_was_written_from():
    got, want = inl.source_statements(), inl.census_statements()
    for key in want:
        assert got[key] == want[key], f"the launch code's {key} changed: update instantiation_lib's census, then this text"


def test_tripwire_trips_on_a_changed_table(tmp_path):
    """a copy of the two files with one clause of the predicate gone, one template argument dropped, one routing flag changed, one
    plane selector, one arm of with_arm and one arm of MODES swapped"""
    texts = {"engine.hip": inl.ENGINE_HIP.read_text(), "tally_kernels.h": inl.KERNELS_H.read_text()}
    for key, name, old, new in (
            ("exists", "tally_kernels.h", " && (DO_PSS || !MASKQ) && (!LATER || pss_alone) &&", " && (!LATER || pss_alone) &&"),
            ("launch_sites", "engine.hip", "tally_tiled_kmer_planes<SEL(), LDS_KMER(), REGIONS()>", "tally_tiled_kmer_planes<SEL(), LDS_KMER()>"),
            ("routing", "engine.hip", "}, kmer_lds, regions);", "}, kmer_lds, false);"),
            ("plane_selectors", "engine.hip", "sel == PLANES_HASH ? f(std::integral_constant<PlaneSel, PLANES_HASH>{})", "sel == PLANES_HASH ? f(std::integral_constant<PlaneSel, PLANES_REF>{})"),
            ("arms", "engine.hip", "arm == ARM_COMP     ? f(std::integral_constant<TallyArm, ARM_COMP>{})", "arm == ARM_COMP     ? f(std::integral_constant<TallyArm, ARM_MISM>{})"),
            ("mode_arms", "engine.hip", '{"the interior table", interior_on, ARM_INTERIOR},', '{"the interior table", interior_on, ARM_MISM},')):
        assert texts[name].count(old) == 1, key
        for n, text in texts.items():
            (tmp_path / n).write_text(text.replace(old, new) if n == name else text)
        got, want = inl.source_statements(tmp_path / "engine.hip", tmp_path / "tally_kernels.h"), inl.census_statements()
        assert [k for k in want if got[k] != want[k]] == [key]


def test_exists_mirror_on_a_few_known_combinations():
    on = lambda **f: inl.exists(*inl.tiled(**f)[1])   # noqa: E731
    assert on(DO_PSS=1) and on(DO_KMER=1) and on(DO_KMER=1, LDS_KMER=1) and not on() and not on(LDS_KMER=1, DO_PSS=1)
    assert on(DO_PSS=1, SITE=1, LATER=1) and not on(DO_PSS=1, HIST=1, LATER=1)
    assert not on(DO_KMER=1, MASKQ=1) and on(DO_KMER=1, REGIONS=1) and not on(DO_PSS=1, DO_KMER=1, SITE=1)
    assert on(DO_PSS=1, GAPPED=1, LATER=1, MASKQ=1, REGIONS=1) and not on(DO_PSS=1, DO_KMER=1, GAPPED=1)
    for one in ("END", "MISM", "INTERIOR", "COMP"):
        assert on(DO_PSS=1, **{one: 1}) and not on(DO_PSS=1, LATER=1, **{one: 1}) and not on(DO_PSS=1, DO_KMER=1, **{one: 1})
    assert on(DO_PSS=1, SCORE=1, MASKQ=1, REGIONS=1) and not on(DO_PSS=1, LATER=1, SCORE=1) and not on(DO_PSS=1, DO_KMER=1, SCORE=1)
    for two in (dict(SITE=1, HIST=1), dict(MISM=1, INTERIOR=1), dict(INTERIOR=1, COMP=1), dict(MISM=1, COMP=1)):      # two options at once: no such instantiation can be written
        with pytest.raises(ValueError):
            inl.tiled(DO_PSS=1, **two)


# ---- instantiations <-> configurations -------------------------------------------------------------------------------------

def test_every_instantiation_has_a_configuration_that_launches_it():
    for fam in inl.enumerate_all().values():
        for inst in fam:
            c = inl.config_of(inst)
            assert inst in inl.launched(c), (inl.describe(inst), c.name)
            if inst not in inl.ELSEWHERE:
                assert c.name in inl.BY_NAME, (inl.describe(inst), c.name)


def test_row_passes():
    """-r 40 launches the pass-0 kernel and the later-pass kernel of the same MASKQ / REGIONS; -r 25 one kernel"""
    for c in inl.CONFIGS:
        got = inl.launched(c)
        later = [i for i in got if (i[0] == "tally_tiled" and i[1][3]) or (i[0] == "tally_tiled_planes" and i[1][1])]
        assert len(got) == (2 if c.r == inl.LONG_R else 1) and len(later) == (1 if c.r == inl.LONG_R else 0), c.name
        if c.r:
            assert (c.r == inl.LONG_R) == (c.option in ("-", "X", "I") or c.family == "planes") or c.family == "compact", c.name
        for kernel, args in got:
            flags = dict(zip(inl.TILED_FLAGS, args)) if kernel == "tally_tiled" else None
            if flags and flags["DO_PSS"]:
                assert flags["MASKQ"] == c.maskq and flags["REGIONS"] == c.regions
            if flags and flags["DO_KMER"]:
                assert flags["LDS_KMER"] == (c.klen == 4)


def test_the_configuration_list_covers_every_instantiation():
    assert len({c.name for c in inl.CONFIGS}) == len(inl.CONFIGS) == 85
    by_family = {}
    for c in inl.CONFIGS:
        by_family[c.family] = by_family.get(c.family, 0) + 1
    assert by_family == {"pss": 32, "pss_kmer": 16, "kmer": 4, "planes": 20, "kmer_planes": 12, "compact": 1}
    covered = set().union(*(inl.launched(c) for c in inl.CONFIGS))
    everything = {i for fam in inl.enumerate_all().values() for i in fam}
    assert covered | set(inl.ELSEWHERE) == everything and not covered & set(inl.ELSEWHERE)
    assert covered - everything == set()
    assert {i for i in everything if i[0] == "tally_compact"} - covered == set(inl.COMPACT_ELSEWHERE)
    assert {i for i in everything if i[0] == "tally_tiled"} - covered == set(inl.SCORE_ELSEWHERE)


def test_the_other_compact_forms_are_launched_where_the_census_says():
    """the ids name arms of test_gpu_tile_loop.COMPACT, and the arm's engine set-up launches that very instantiation"""
    for inst, test_id in inl.COMPACT_ELSEWHERE.items():
        arm = test_id[test_id.index("[") + 1:].split("-")[0]
        assert test_id.startswith("test_gpu_tile_loop.py::test_compact_walks_several_tiles[") and arm in COMPACT
        parts = arm.split("_")
        r = int(next(p for p in parts if p.startswith("r"))[1:])
        k = next((int(p[1:]) for p in parts if p.startswith("k")), None)
        assert inl.launched(inl.Config("compact", "-", r, k, plan_once=arm.startswith("plan_once"))) == {inst}


def test_the_score_forms_are_launched_where_the_census_says():
    """the ids name tests of test_gpu_read_score, and the engine set-up of each (its check_filter call: -r, -Q, -T and the tiled
    kernel) launches that very instantiation"""
    assert len(inl.SCORE_ELSEWHERE) == len(set(inl.SCORE_ELSEWHERE.values())) == 4
    for inst, test_id in inl.SCORE_ELSEWHERE.items():
        name, param = re.fullmatch(r"test_gpu_read_score\.py::(\w+)\[(\w+)\]", test_id).groups()
        src = inspect.getsource(getattr(test_gpu_read_score, name))
        assert (param == "TILED" and "TILED" in test_gpu_read_score.KERNELS) or test_gpu_read_score.SHAPES[param].get("PSSBAM_GRID_WGS")
        (r,), (call,) = re.findall(r"PssOpts\(region_len=(\d+)\)", src), re.findall(r"check_filter\(pkg, \w+, o, kernel, ([^\n]*)\)\n", src)
        c = inl.Config("pss", "Y", int(r), None, maskq="q=q" in call, regions="ivs=ivs" in call)
        assert inl.launched(c) == {inst}, test_id


# ---- the expectations -------------------------------------------------------------------------------------------------------

def rows_differ(a, b) -> bool:
    return bool((a[0][2:] != b[0][2:]).any() and (a[1][2:] != b[1][2:]).any())


def ok_of(arm, c) -> int:
    return arm.want["stats"]["pss_ok" if c.r else "kmer_ok"]


def test_every_configuration_has_an_expectation(built):
    D, A = built
    assert set(A) == set(inl.BY_NAME) and set(inl.TILED_CONFIGS) | set(inl.COMPACT_CONFIGS) == set(A)
    for name, arm in A.items():
        c = inl.BY_NAME[name]
        assert arm.data == c.data and (arm.regions is not None) == c.regions and arm.kw == c.kw and arm.env == c.env
        assert ("tables" in arm.want) == bool(c.r) and ("kmer" in arm.want) == bool(c.klen) and arm.want["stats"]["records"] == inl.N_READS
        for t in arm.want.get("tables", ()):
            assert t.shape == (c.r + 2, 16) and t[2:].any() and t[:2].any()
        for t in arm.want.get("kmer", ()):
            assert t.any()


def test_base_quality_mask_bites(built):
    _, A = built
    for c in inl.CONFIGS:
        if c.maskq:
            assert rows_differ(A[c.name].want["tables"], A[c.twin(maskq=False).name].want["tables"]), c.name
            if c.klen:      # the k-mer tables do not depend on -Q
                assert all(np.array_equal(a, b) for a, b in zip(A[c.name].want["kmer"], A[c.twin(maskq=False).name].want["kmer"]))


def test_regions_keep_some_reads_and_drop_some(built):
    _, A = built
    for c in inl.CONFIGS:
        if c.regions:
            whole = A[c.twin(regions=False).name]
            assert 0 < ok_of(A[c.name], c) < ok_of(whole, c), c.name
            if c.r and c.klen:
                assert 0 < A[c.name].want["stats"]["kmer_ok"] < whole.want["stats"]["kmer_ok"], c.name


def test_both_filters_together_differ_from_either(built):
    _, A = built
    for c in inl.CONFIGS:
        if c.maskq and c.regions:
            mine = A[c.name].want["tables"]
            assert rows_differ(mine, A[c.twin(regions=False).name].want["tables"]) and rows_differ(mine, A[c.twin(maskq=False).name].want["tables"]), c.name


def test_planes_are_populated(built):
    _, A = built
    seen = 0
    for c in inl.CONFIGS:
        if c.family not in ("planes", "kmer_planes"):
            continue
        want = A[c.name].want
        planes = want["replicates"] if "replicates" in want else list(want["contigs"].values()) if "contigs" in want else None
        if planes is None:
            kind, by_key = want["planes"]
            planes = list(by_key.values())
            if kind == "groups":        # plane 0: the reads of no listed group
                assert list(by_key)[0] is None
            elif kind == "sets":        # plane 0: what the totals hold beyond the sets
                total = want["tables"] if c.r else want["kmer"]
                rest = [total[s].astype(np.int64) - sum(p[s].astype(np.int64) for p in planes) for s in (0, 1)]
                assert all((x >= 0).all() for x in rest)
                planes = [rest] + planes
        body = (lambda t: t[2:]) if c.r else (lambda t: t)
        full = [bool(body(p[0]).any() and body(p[1]).any()) for p in planes]
        assert full[0] and sum(full) >= 2, (c.name, full)
        seen += 1
    assert seen == 32


def test_the_later_row_pass_has_rows_to_add(built):
    _, A = built
    for c in inl.CONFIGS:
        if c.r == inl.LONG_R:
            f, r = A[c.name].want["tables"]
            assert f[34:].any() and r[34:].any(), c.name
            for pf, pr in A[c.name].want.get("site", ()):
                assert pf[34:].any() and pr[34:].any(), c.name


def test_every_feature_table_is_non_zero_on_both_strands(built):
    _, A = built
    seen = {}
    for c in inl.CONFIGS:
        want = A[c.name].want
        for key in ("hist", "site", "end", "mism", "interior", "composition"):
            if key not in want:
                continue
            seen[key] = seen.get(key, 0) + 1
            if key == "site":
                assert all(t[2:].any() for pair in want["site"] for t in pair), c.name
            elif key == "end":
                cf, cr, reads = want["end"]
                assert cf[2:].any() and cr[2:].any() and reads[0] > reads[1] > 0 and reads[0] > reads[2] > 0, (c.name, reads)
            elif key == "interior":
                fwd, rev = want["interior_by_strand"]
                assert fwd[0].any() and rev[0].any() and fwd[1] > 0 and rev[1] > 0 and want["interior"][0][[1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14]].all(), c.name
            else:
                assert want[key][0].any() and want[key][1].any() and not np.array_equal(want[key][0], want[key][1]), (c.name, key)
    assert seen == {"hist": 12, "site": 4, "end": 4, "mism": 4, "interior": 4, "composition": 4}


def test_interior_expectation_depends_on_base_quality_and_composition_does_not(built):
    _, A = built
    for t in (False, True):
        w = {q: A[inl.Config("pss", "W", inl.SHORT_R, None, q, t).name].want["interior"] for q in (False, True)}
        assert w[True][1] == w[False][1] and 0 < int(w[True][0].sum()) < int(w[False][0].sum())
        p = {q: A[inl.Config("pss", "P", inl.SHORT_R, None, q, t).name].want["composition"] for q in (False, True)}
        assert all(np.array_equal(a, b) for a, b in zip(p[True], p[False]))


def test_datasets_keep_the_launch_shapes_honest(built):
    """every workgroup walks at least five tiles in both shapes (assert_every_tile_overflows ran in datasets())"""
    D, _ = built
    assert set(D) == {"plain", "sets", "rg", "dmg", "gap"}
    for wgs, tile in ((3, 48), (2, 64)):
        assert -(-inl.N_READS // tile) // wgs >= 5

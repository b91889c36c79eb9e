"""The census of the tiled tally family: every kernel instantiation the engine can launch, the Engine configuration that
launches each, and the CPU expectation of every configuration.  Shared by test_instantiations_host.py (no GPU) and
test_gpu_instantiations.py.

launch_tally / launch_tiled (pss-bam_amd/csrc/engine.hip) turn runtime flags and the engine's arm (TallyArm: the one of
the options -H -X -E -I -n/-N -W -P -y/-Y that is on) into template arguments; every combination is a kernel of its own,
with its own registers and spills.  `exists` below mirrors the predicate tally_tiled_exists of tally_kernels.h;
EXISTS_SOURCE, LAUNCH_SITES, GUARDS, ROUTING, ARMS and MODE_ARMS are the statements of the two files the mirror and
`launched` were written from, whitespace-normalised, and source_statements() reads them back from the files: when they
differ the instantiation table has changed, and the census (the mirror, `launched`, the counts and the configuration
list) has to follow before the texts are updated.

An instantiation is (kernel name, template arguments); a Config is one engine set-up; launched(cfg) is the set of
instantiations its launches go through, config_of(inst) a configuration that launches a given one.  CONFIGS is the list
test_gpu_instantiations.py runs: 32 pss-only, 16 pss + k-mer, 4 k-mer-only, 20 plane, 12 k-mer-plane configurations and
the one tally_compact form test_gpu_tile_loop.py does not launch.  The other five compact forms are COMPACT_ELSEWHERE,
the four tally_tiled forms of the SCORE arm (-y / -Y) SCORE_ELSEWHERE, both by test id.

Expectations are composed the way the arms' own feature tests build them: records -> regions_lib.reduce_recs (-T) ->
base_quality_lib.mask_recs (-Q 20) -> the feature's expectation (the CPU oracle, or the feature lib's direct count).
-n and -I are the two features whose own tests put a step in front: the mismatch count is taken from SEQ as stored and
the anchoring from the record as stored, so reduce_to / anchor_recs come first.  The k-mer tables, -H's rows and -P's
blocks do not look at base qualities.  Datasets, seeds, Arm, Data and the stats helpers are test_gpu_tile_loop's."""
from __future__ import annotations

import itertools
import re
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import base_quality_lib as bq
import composition_lib as cl
import end_condition_lib as ec
import gapped_lib as gl
import interior_lib as il
import mismatch_lib as ml
import pssbam_testlib as tl
import regions_lib as rl
import replicates_lib as rp
import site_context_lib as sc
from test_gpu_contig_sets import oracle_sets
from test_gpu_kmer_planes import oracle_on_contigs
from test_gpu_length_bins import bins_of, oracle_bins
from test_gpu_length_disagree import mism_hist
from test_gpu_per_contig import oracle_planes
from test_gpu_read_groups import first_rg
from test_gpu_tile_loop import (CONTIG_SETS, END_COND, HIST_MAX, KMER_EDGES, LEN_EDGES, N_READS, RG_IDS, Arm, Data,
                                assert_every_tile_overflows, direct_hist, region_stats, sam_of, stats_of)

ENGINE_HIP = Path(__file__).resolve().parent.parent / "pss-bam_amd" / "csrc" / "engine.hip"
KERNELS_H = ENGINE_HIP.parent / "tally_kernels.h"

# ---- the statements of engine.hip and tally_kernels.h this census was written from (the tripwire) -----------------------

EXISTS_SOURCE = (
    "constexpr bool tally_tiled_exists(bool DO_PSS, bool DO_KMER, bool LDS_KMER, bool LATER, bool MASKQ, TallyArm ARM) { "
    "const bool pss_alone = DO_PSS && !DO_KMER; "
    "return (DO_PSS || DO_KMER) && (DO_KMER || !LDS_KMER) && (DO_PSS || !MASKQ) && (!LATER || pss_alone) && "
    "(ARM == ARM_NONE || (ARM == ARM_HIST ? DO_PSS && !LATER : ARM == ARM_SITE || ARM == ARM_GAPPED ? pss_alone : pss_alone && !LATER)); }")

# every `kernel<template arguments>` of the four kernels in engine.hip, in file order
LAUNCH_SITES = [
    "tally_tiled<DO_PSS(), DO_KMER(), LDS_KMER(), LATER(), MASKQ(), REGIONS(), ARM()>",
    "tally_tiled_planes<PLANES_EACH, LATER(), MASKQ(), REGIONS()>",
    "tally_tiled_planes<SEL(), LATER(), MASKQ(), REGIONS()>",
    "tally_tiled_kmer_planes<SEL(), LDS_KMER(), REGIONS()>",
    "tally_compact<DO_KMER(), LDS_KMER(), PLAN_ONCE()>",
]
# every `if constexpr (...)` between launch_tiled and the end of launch_tally, and the selectors with_planes knows
GUARDS = ["tally_tiled_exists(DO_PSS(), DO_KMER(), LDS_KMER(), LATER(), MASKQ(), ARM())", "SEL() == PLANES_HASH", "SEL() == PLANES_HASH",
          "DO_KMER() || !LDS_KMER()"]
PLANE_SELECTORS = ["PLANES_RG", "PLANES_LEN", "PLANES_HASH", "PLANES_REF"]      # (PLANES_EACH has a launch site of its own)
# the arms with_arm knows, and the arm column of MODES (five plane modes, then -H -X -E -I -n/-N -W -P -y/-Y)
ARMS = ["ARM_HIST", "ARM_SITE", "ARM_END", "ARM_GAPPED", "ARM_MISM", "ARM_INTERIOR", "ARM_COMP", "ARM_SCORE", "ARM_NONE"]
MODE_ARMS = ["ARM_NONE"] * 5 + ARMS[:8]
# the runtime flags behind the template arguments, and which launch a block takes
ROUTING = [
    "}, do_pss, do_kmer, kmer_lds, later, maskq, regions);",
    "}, pass > 0, maskq, regions);",
    "}, pass > 0, maskq, regions);",
    "}, kmer_lds, regions);",
    "}, do_kmer, kmer_lds, e->compact_plan_once);",
    "} else if (do_pss && e->rows <= COMPACT_MAX_ROWS && e->use_compact && !e->has_rg && !maskq && !regions && arm == ARM_NONE) {",
    "const TallyArm later_arm = arm == ARM_SITE || arm == ARM_GAPPED ? arm : ARM_NONE;",
    "rc = pass == 0 ? launch_tiled(e, P, do_pss, do_kmer, kmer_lds, false, maskq, regions, arm, lds0, n_tiles) "
    ": launch_tiled(e, P, true, false, false, true, maskq, regions, later_arm, lds, n_tiles);",
]
CONSTANTS = {"TILED_ROWS": 32, "KMER_LDS_MAX_K": 4, "COMPACT_MAX_ROWS": 18}      # tally_kernels.h


def _norm(text: str) -> str:
    return " ".join(text.split())


def source_statements(engine: Path = ENGINE_HIP, kernels: Path = KERNELS_H) -> dict:
    """the same statements read from engine.hip and tally_kernels.h, whitespace-normalised"""
    text, ktext = engine.read_text(), kernels.read_text()
    region = text[text.index("static int launch_tiled("):text.index('extern "C" int pssbam_engine_hint_records')]
    planes_fn = text[text.index("static int with_planes("):text.index("static int no_kernel()")]
    routing = [m.group(0) for m in re.finditer(r"^\s*\}, [^\n{}]*\);$", region, re.M)]
    routing += re.findall(r"\} else if \(do_pss && e->rows <= COMPACT_MAX_ROWS[^{]*\{", region)
    routing += re.findall(r"const TallyArm later_arm = [^;]*;", region)
    routing += re.findall(r"rc = pass == 0 \? launch_tiled\(.*?;\n", region, re.S)
    return {
        "exists": [_norm(m) for m in re.findall(r"constexpr bool tally_tiled_exists\(.*?\n\}", ktext, re.S)],
        "launch_sites": [_norm(m.group(0)) for m in re.finditer(r"\b(?:tally_tiled|tally_tiled_planes|tally_tiled_kmer_planes|tally_compact)<[^<>;]*>", text)],
        "guards": [_norm(m) for m in re.findall(r"if constexpr \((.*?)\)(?= return|$)", region, re.M)],
        "plane_selectors": re.findall(r"integral_constant<PlaneSel, (PLANES_\w+)>", planes_fn),
        "arms": re.findall(r"integral_constant<TallyArm, (ARM_\w+)>", text),
        "mode_arms": re.findall(r'^\s*\{"[^"]*", .*, (ARM_\w+)\},$', text, re.M),
        "routing": [_norm(s) for s in routing],
        "constants": tl_constants(ktext),
    }


def tl_constants(text: str) -> dict:
    return {k: int(re.search(rf"constexpr \w+ {k} = (\d+);", text).group(1)) for k in CONSTANTS}


def census_statements() -> dict:
    return {"exists": [EXISTS_SOURCE], "launch_sites": LAUNCH_SITES, "guards": GUARDS, "plane_selectors": PLANE_SELECTORS, "arms": ARMS,
            "mode_arms": MODE_ARMS, "routing": [_norm(s) for s in ROUTING], "constants": CONSTANTS}


# ---- the instantiations ---------------------------------------------------------------------------------------------------

TILED_FLAGS = ("DO_PSS", "DO_KMER", "LDS_KMER", "LATER", "MASKQ", "REGIONS", "ARM")      # six bools and the arm, "NONE" or an OPTION_ARM value
OPTION_ARM = {"H": "HIST", "X": "SITE", "E": "END", "I": "GAPPED", "N": "MISM", "W": "INTERIOR", "P": "COMP", "Y": "SCORE"}
PLANES = ("RG", "LEN", "HASH", "REF", "EACH")           # -G, -S, -J, -C, -A
KMER_PLANES = ("RG", "LEN", "REF")
COUNTS = {"tally_tiled": 68, "tally_tiled_planes": 40, "tally_tiled_kmer_planes": 12, "tally_compact": 6}


def exists(DO_PSS, DO_KMER, LDS_KMER, LATER, MASKQ, REGIONS, ARM) -> bool:
    """tally_tiled_exists (EXISTS_SOURCE), clause by clause; REGIONS is free"""
    pss_alone = DO_PSS and not DO_KMER
    return bool(
        (DO_PSS or DO_KMER) and (DO_KMER or not LDS_KMER) and (DO_PSS or not MASKQ) and (not LATER or pss_alone)
        and (ARM == "NONE" or ((DO_PSS and not LATER) if ARM == "HIST" else pss_alone if ARM in ("SITE", "GAPPED") else (pss_alone and not LATER))))


def tiled(**on) -> tuple:
    """the tally_tiled instantiation with the named flags on; an arm is named like a flag, and two arms are refused"""
    arms = [a for a in OPTION_ARM.values() if on.pop(a, 0)]
    if len(arms) > 1:
        raise ValueError(f"one arm per instantiation, not {arms}")
    assert set(on) <= set(TILED_FLAGS[:6])
    return ("tally_tiled", tuple(int(bool(on.get(f, 0))) for f in TILED_FLAGS[:6]) + ((arms or ["NONE"])[0],))


def enumerate_all() -> dict:
    """{kernel: [instantiation]} of the four families"""
    return {
        "tally_tiled": [("tally_tiled", bits + (arm,)) for bits in itertools.product((0, 1), repeat=6) for arm in ["NONE", *OPTION_ARM.values()]
                        if exists(*bits, arm)],
        "tally_tiled_planes": [("tally_tiled_planes", (sel, later, maskq, regions))
                               for sel in PLANES for later in (0, 1) for maskq in (0, 1) for regions in (0, 1)],
        "tally_tiled_kmer_planes": [("tally_tiled_kmer_planes", (sel, lds, regions)) for sel in KMER_PLANES for lds in (0, 1) for regions in (0, 1)],
        "tally_compact": [("tally_compact", (do_kmer, lds, once)) for do_kmer, lds in ((0, 0), (1, 0), (1, 1)) for once in (0, 1)],
    }


def describe(inst) -> str:
    """`tally_tiled<DO_PSS, MASKQ, SITE>` (the flags that are on and the arm), `tally_tiled_planes<LEN, LATER=1, MASKQ=0, REGIONS=1>`, ..."""
    kernel, args = inst
    if kernel == "tally_tiled":
        return f"tally_tiled<{', '.join([f for f, b in zip(TILED_FLAGS, args[:6]) if b] + [a for a in args[6:] if a != 'NONE'])}>"
    names = {"tally_tiled_planes": ("", "LATER=", "MASKQ=", "REGIONS="), "tally_tiled_kmer_planes": ("", "LDS_KMER=", "REGIONS="),
             "tally_compact": ("DO_KMER=", "LDS_KMER=", "PLAN_ONCE=")}[kernel]
    return f"{kernel}<{', '.join(f'{n}{a}' for n, a in zip(names, args))}>"


# ---- the configurations ---------------------------------------------------------------------------------------------------

MIN_BQ = 20
MISM = (10, 3, 0)           # -N 10 -n 3
INTERIOR_MARGIN = 5
COMPOSITION = 10
REPLICATES = 5
LONG_R, SHORT_R = 40, 25    # two row passes / one (-H, -E, -n, -W and -P need -r <= 30 or belong to pass 0)
OPTION_KW = {"-": {}, "H": dict(length_hist=HIST_MAX), "X": dict(site_context="cpg"), "E": dict(end_condition=END_COND), "I": dict(gapped=True),
             "N": dict(mismatches=MISM), "W": dict(interior=INTERIOR_MARGIN), "P": dict(composition=COMPOSITION)}
PLANE_KW = {"RG": dict(read_groups=RG_IDS), "LEN": dict(length_bins=LEN_EDGES[LONG_R]), "HASH": dict(replicates=REPLICATES),
            "REF": dict(contig_sets=CONTIG_SETS), "EACH": dict(per_contig=True)}
KMER_PLANE_KW = {"RG": dict(read_groups=RG_IDS), "LEN": dict(length_bins=KMER_EDGES), "REF": dict(contig_sets=CONTIG_SETS)}
DATA_OF = {"E": "dmg", "I": "gap", "RG": "rg", "REF": "sets", "EACH": "sets"}
REGION_SEED = {"plain": 9601, "sets": 9602, "rg": 9603, "dmg": 9604, "gap": 9606}
# regions_lib.fuzz_intervals covers chrB and chrA alone: with these the unassigned contig of -C and its smallest set keep reads under -T
MORE_REGIONS = {"sets": [("scaffold_10", 0, 150), ("tiny.4", 200, 600)]}


@dataclass(frozen=True)
class Config:
    family: str             # pss | pss_kmer | kmer | planes | kmer_planes | compact
    option: str = "-"       # - H X E I N W P, or the plane selector
    r: int | None = None    # -r (None: no substitution tally)
    klen: int | None = None
    maskq: bool = False     # -Q 20
    regions: bool = False   # -T
    plan_once: bool = False

    @property
    def name(self) -> str:
        parts = [self.family, self.option] + ([f"r{self.r}"] if self.r else []) + ([f"k{self.klen}"] if self.klen else [])
        return "_".join(parts + ["Q"] * self.maskq + ["T"] * self.regions + ["once"] * self.plan_once)

    @property
    def data(self) -> str:
        return DATA_OF.get(self.option, "plain")

    @property
    def kw(self) -> dict:
        """the Engine keyword arguments (kernel excepted)"""
        kw = dict(pss=dict(region_len=self.r) if self.r else None, kmer=dict(klen=self.klen) if self.klen else None)
        if self.maskq:
            kw["min_base_qual"] = MIN_BQ
        kw.update(PLANE_KW[self.option] if self.family == "planes" else KMER_PLANE_KW[self.option] if self.family == "kmer_planes"
                  else OPTION_KW[self.option])
        return kw

    @property
    def env(self) -> dict:
        return {"PSSBAM_COMPACT_PLAN_ONCE": "1"} if self.plan_once else {}

    def twin(self, **change) -> "Config":
        return Config(**{**self.__dict__, **change})


def launched(c: Config) -> set:
    """launch_tally under KERNEL_AUTO: the instantiations one submit of this configuration goes through"""
    do_pss, do_kmer = c.r is not None, c.klen is not None
    maskq, regions = int(do_pss and c.maskq), int(c.regions)
    kmer_lds = int(do_kmer and c.klen <= CONSTANTS["KMER_LDS_MAX_K"])
    rows = c.r + 2 if do_pss else 0
    n_passes = -(-rows // CONSTANTS["TILED_ROWS"]) if do_pss else 1
    if c.family in ("planes", "kmer_planes"):
        if do_pss:
            return {("tally_tiled_planes", (c.option, int(p > 0), maskq, regions)) for p in range(n_passes)}
        return {("tally_tiled_kmer_planes", (c.option, kmer_lds, regions))}
    arm = OPTION_ARM.get(c.option) if do_pss else None
    if do_pss and rows <= CONSTANTS["COMPACT_MAX_ROWS"] and not maskq and not regions and arm is None:
        return {("tally_compact", (int(do_kmer), kmer_lds, int(c.plan_once)))}
    out = {tiled(DO_PSS=do_pss, DO_KMER=do_kmer, LDS_KMER=kmer_lds, MASKQ=maskq, REGIONS=regions, **({arm: 1} if arm else {}))}
    if n_passes > 1:
        out.add(tiled(DO_PSS=1, LATER=1, MASKQ=maskq, REGIONS=regions, **({arm: 1} if arm in ("SITE", "GAPPED") else {})))
    return out


def config_of(inst) -> Config:
    """a configuration whose launches include the instantiation"""
    kernel, args = inst
    if kernel == "tally_tiled_planes":
        sel, _, maskq, regions = args
        return Config("planes", sel, LONG_R, None, bool(maskq), bool(regions))
    if kernel == "tally_tiled_kmer_planes":
        sel, lds, regions = args
        return Config("kmer_planes", sel, None, 4 if lds else 6, False, bool(regions))
    if kernel == "tally_compact":
        do_kmer, lds, once = args
        return Config("compact", "-", 15, (4 if lds else 9) if do_kmer else None, plan_once=bool(once))
    f = dict(zip(TILED_FLAGS, args))
    option = next((o for o, arm in OPTION_ARM.items() if f["ARM"] == arm), "-")
    klen = (4 if f["LDS_KMER"] else 9) if f["DO_KMER"] else None
    if not f["DO_PSS"]:
        return Config("kmer", "-", None, klen, False, bool(f["REGIONS"]))
    r = LONG_R if option in ("-", "X", "I") else SHORT_R
    return Config("pss_kmer" if klen else "pss", option, r, klen, bool(f["MASKQ"]), bool(f["REGIONS"]))


QT = [(q, t) for t in (False, True) for q in (False, True)]
CONFIGS = ([Config("pss", o, LONG_R if o in ("-", "X", "I") else SHORT_R, None, q, t) for o in OPTION_KW for q, t in QT]
           + [Config("pss_kmer", o, LONG_R if o == "-" else SHORT_R, k, q, t) for o in ("-", "H") for k in (4, 9) for q, t in QT]
           + [Config("kmer", "-", None, k, False, t) for k in (4, 9) for t in (False, True)]
           + [Config("planes", sel, LONG_R, None, q, t) for sel in PLANES for q, t in QT]
           + [Config("kmer_planes", sel, None, k, False, t) for sel in KMER_PLANES for k in (4, 6) for t in (False, True)]
           + [Config("compact", "-", 15, 9, plan_once=True)])
BY_NAME = {c.name: c for c in CONFIGS}
TILED_CONFIGS = [c.name for c in CONFIGS if c.family != "compact"]
COMPACT_CONFIGS = [c.name for c in CONFIGS if c.family == "compact"]

# the compact forms another module launches, by test id (shape three_wg; the other NO_XCD shapes run them too)
COMPACT_ELSEWHERE = {
    ("tally_compact", (0, 0, 0)): "test_gpu_tile_loop.py::test_compact_walks_several_tiles[compact_r16-three_wg]",
    ("tally_compact", (1, 0, 0)): "test_gpu_tile_loop.py::test_compact_walks_several_tiles[compact_r16_k9-three_wg]",
    ("tally_compact", (1, 1, 0)): "test_gpu_tile_loop.py::test_compact_walks_several_tiles[compact_r16_k4-three_wg]",
    ("tally_compact", (0, 0, 1)): "test_gpu_tile_loop.py::test_compact_walks_several_tiles[plan_once_r15-three_wg]",
    ("tally_compact", (1, 1, 1)): "test_gpu_tile_loop.py::test_compact_walks_several_tiles[plan_once_r15_k4-three_wg]",
}


# the four forms of the SCORE arm (-y / -Y: without and with -Q and -T), by the test of test_gpu_read_score.py that launches each
SCORE_ELSEWHERE = {
    tiled(DO_PSS=1, SCORE=1): "test_gpu_read_score.py::test_several_tiles_per_workgroup[three_wg]",
    tiled(DO_PSS=1, SCORE=1, MASKQ=1): "test_gpu_read_score.py::test_filter_with_min_base_quality[TILED]",
    tiled(DO_PSS=1, SCORE=1, REGIONS=1): "test_gpu_read_score.py::test_filter_with_regions[TILED]",
    tiled(DO_PSS=1, SCORE=1, MASKQ=1, REGIONS=1): "test_gpu_read_score.py::test_filter_with_min_base_quality_and_regions[TILED]",
}
ELSEWHERE = {**COMPACT_ELSEWHERE, **SCORE_ELSEWHERE}


# ---- the expectations (CPU only) ------------------------------------------------------------------------------------------

def kmer_stats(n_records: int, kplain, kred=None) -> dict:
    """the counters of a k-mer-only engine from the oracle's fragkon run on the input (and, with -T, on the reduced input: a
    candidate that meets no region leaves KMER_OK / KMER_FAIL and is FILTERED, test_gpu_regions.check_stats)"""
    out = stats_of(n_records, kplain, kplain, pss=False)
    if kred is not None:
        done = lambda st: int(st[tl.ST_OK] + st[tl.ST_KMER_FAIL])   # noqa: E731
        out.update(kmer_ok=int(kred[tl.ST_OK]), kmer_fail=int(kred[tl.ST_KMER_FAIL]), kmer_filtered=int(kplain[tl.ST_FILTERED]) + done(kplain) - done(kred))
    return out


def datasets() -> dict:
    """test_gpu_tile_loop's five datasets, from its seeds"""
    D = {"plain": Data(*tl.fuzz_dataset(9601, N_READS)),
         "sets": Data(*tl.fuzz_dataset(9602, N_READS, contig_lens=(5000, 1200, 300, 900))),
         "rg": Data(*tl.fuzz_dataset(9603, N_READS, with_rg=True))}
    c, f, r = tl.fuzz_dataset(9604, N_READS)
    D["dmg"] = Data(c, f, ec.plant_damage(c, r, np.random.default_rng(9605), 0.5))
    D["gap"] = Data(*gl.fuzz_case(9606, N_READS)[:3])
    for d in D.values():
        assert len(d.recs) == N_READS
        assert_every_tile_overflows(d.raw)
    return D


class Builder:
    """the oracle runs of one dataset, each made once"""

    def __init__(self, oracle, tmp, key: str, d: Data):
        self.oracle, self.tmp, self.key, self.d = oracle, tmp, key, d
        self.g = oracle.genome_from_arrays(d.loaded)
        self.ivs = rl.fuzz_intervals(REGION_SEED[key], d.contigs, d.recs) + MORE_REGIONS.get(key, [])
        self._memo = {}
        self._n = 0

    def close(self):
        self.oracle.free_genome(self.g)

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def sam(self, recs):
        self._n += 1
        return sam_of(self.tmp, f"{self.key}_{self._n}.sam", self.d.refs, recs)

    def recs(self, q: bool, t: bool, first=None) -> list:
        """records -> `first` (the feature's own step on the records as stored) -> -T -> -Q"""
        def make():
            out = self.d.recs if first is None else self.memo(("first", first), lambda: FIRST[first](self.d))
            out = rl.reduce_recs(out, self.ivs) if t else out
            return bq.mask_recs(out, MIN_BQ) if q else out
        return self.memo(("recs", q, t, first), make)

    def pss(self, r: int, q: bool, t: bool, first=None):
        return self.memo(("pss", r, q, t, first), lambda: self.oracle.pss(self.g, self.sam(self.recs(q, t, first)), tl.PssOpts(region_len=r)))

    def fragkon(self, k: int, t: bool, **more):
        """(the k-mer tally never looks at a base quality)"""
        return self.memo(("fk", k, t, tuple(more.items())), lambda: self.oracle.fragkon(self.g, self.sam(self.recs(False, t)), tl.FkOpts(klen=k, **more)))


FIRST = {"mism": lambda d: ml.reduce_to(d.recs, d.contigs, MISM[1], bool(MISM[2])),     # m is taken from SEQ as stored
         "anchor": lambda d: gl.anchor_recs(d.recs)}                                    # the filler carries quality 0; -T sees the span


def expectation(b: Builder, c: Config) -> Arm:
    """one configuration's Arm: Engine arguments, -T intervals and everything test_gpu_tile_loop.check compares"""
    d, q, t = b.d, c.maskq, c.regions
    want: dict = {}
    first = {"N": "mism", "I": "anchor"}.get(c.option) if c.family in ("pss", "pss_kmer") else None
    if c.r:
        o = tl.PssOpts(region_len=c.r)
        wf, wr, st = b.pss(c.r, q, t, first)
        want["tables"] = (wf, wr)
        base = b.pss(c.r, False, False, "anchor" if first == "anchor" else None)[2]     # the counters without -T (and without -n)
        want["stats"] = region_stats(N_READS, base, st) if (t or first == "mism") else stats_of(N_READS, st)
        plain_recs = b.recs(False, t)                                                    # what the quality-blind features count
    if c.klen:
        k5, k3, kst = b.fragkon(c.klen, t)
        want["kmer"] = (k5, k3)
        kplain = b.fragkon(c.klen, False)[2]
        if c.r:
            want["stats"] = region_stats(N_READS, b.pss(c.r, False, False)[2], st, kplain, kst) if t else stats_of(N_READS, st, kst)
        else:
            want["stats"] = kmer_stats(N_READS, kplain, kst if t else None)
    if c.family in ("pss", "pss_kmer"):
        if c.option == "H":
            by_class = b.memo(("hist", t), lambda: direct_hist(d.contigs, plain_recs, o, HIST_MAX))
            want["hist"] = (sum(v[0] for v in by_class.values()), sum(v[1] for v in by_class.values()))
        elif c.option == "X":
            want["site"] = tuple(b.memo(("site", q, t, keep), lambda: b.oracle.pss(b.g, b.sam(sc.mask_recs(d.contigs, b.recs(q, t), keep)), o)[:2])
                                 for keep in (True, False))
        elif c.option == "E":
            want["end"] = ec.expected(b.oracle, b.g, b.tmp, d.refs, d.contigs, plain_recs, o, *END_COND, min_bq=MIN_BQ if q else 0,
                                      mask=(lambda part: bq.mask_recs(part, MIN_BQ)) if q else None)
        elif c.option == "N":
            want["mism"] = b.memo(("mism", t), lambda: mism_hist(b.oracle, b.g, b.tmp, d.refs, d.contigs, plain_recs, o, MISM[0], MISM[1], bool(MISM[2])))
        elif c.option == "W":
            halves = [il.interior([x for x in plain_recs if bool(x.flag & 0x10) == rev], d.contigs, INTERIOR_MARGIN, o, MIN_BQ if q else 0) for rev in (False, True)]
            want["interior"] = (halves[0][0] + halves[1][0], halves[0][1] + halves[1][1])
            want["interior_by_strand"] = halves
            assert halves[0][2] + halves[1][2] == want["stats"]["pss_ok"]
        elif c.option == "P":
            want["composition"] = b.memo(("comp", t), lambda: cl.composition(plain_recs, d.contigs, COMPOSITION, o))[:2]
    elif c.family == "planes":
        recs = b.recs(q, t)
        if c.option == "LEN":
            want["planes"] = ("bins", oracle_bins(b.oracle, b.g, b.sam(recs), o, LEN_EDGES[c.r]))
            assert list(want["planes"][1]) == bins_of(o, LEN_EDGES[c.r])
        elif c.option == "HASH":
            want["replicates"] = [b.oracle.pss(b.g, b.sam(rp.reduce(recs, REPLICATES, j)), o)[:2] for j in range(REPLICATES)]
        elif c.option == "RG":
            want["planes"] = ("groups", {key: b.oracle.pss(b.g, b.sam([x for x in recs if (first_rg(x) == key if key is not None else first_rg(x) not in RG_IDS)]), o)[:2]
                                         for key in [None] + RG_IDS})
        elif c.option == "REF":
            want["planes"] = ("sets", oracle_sets(b.oracle, d.contigs, b.sam(recs), o, CONTIG_SETS))
        else:
            want["contigs"] = oracle_planes(b.oracle, d.contigs, d.refs, b.sam(recs), o)
    elif c.family == "kmer_planes":
        recs, fo = b.recs(False, t), tl.FkOpts(klen=c.klen)
        if c.option == "LEN":
            want["planes"] = ("bins", {(lo, hi): b.fragkon(c.klen, t, min_read_len=lo, max_read_len=hi)[:2] for lo, hi in bins_of(fo, KMER_EDGES)})
        elif c.option == "RG":
            want["planes"] = ("groups", {key: b.oracle.fragkon(b.g, b.sam([x for x in recs if (first_rg(x) == key if key is not None else first_rg(x) not in RG_IDS)]), fo)[:2]
                                         for key in [None] + RG_IDS})
        else:
            sam = b.sam(recs)
            want["planes"] = ("sets", {label: oracle_on_contigs(b.oracle, d.contigs, names, sam, fo) for label, names in CONTIG_SETS.items()})
    return Arm(c.data, c.kw, want, env=c.env, regions=b.ivs if t else None)


def build_arms(oracle, tmp, configs=CONFIGS):
    """-> (datasets, {configuration name: Arm}).  Nothing here touches a GPU."""
    D, A = datasets(), {}
    for key, d in D.items():
        b = Builder(oracle, tmp, key, d)
        try:
            for c in configs:
                if c.data == key:
                    A[c.name] = expectation(b, c)
        finally:
            b.close()
    return D, A

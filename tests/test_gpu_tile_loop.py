"""Every arm of the tally kernels in workgroups that walk SEVERAL tiles, against the oracle.

The tiled family (tally_tiled and its -Q / -T / -H / -X / -E / -I instantiations, tally_tiled_planes,
tally_tiled_kmer_planes, tally_compact) shares one software pipeline over a workgroup's tiles: two offset buffers swapped
by the parity of the trip, a staging buffer refilled for the next tile while the current one is still being tallied,
offsets of the tile after that held in registers, tally_compact's per-tile overflow queue, and LDS tables that must survive
the whole loop.  None of it runs when a workgroup owns one tile, which is the shape of a few thousand records on the
default grid.  Here the grid is shrunk instead (PSSBAM_GRID_WGS, PSSBAM_TILE_READS), so that 3 200 records are 67 tiles of
48 (or 50 of 64) walked by 1, 2, 3, 8 or 16 workgroups; PSSBAM_XCD_MAP=1 changes which tiles a workgroup walks; and the
lane-per-read kernels run in ONE block (PSSBAM_SIMPLE_BLOCKS=1), 13 trips of their grid-stride loop.

Each arm's expectation is built once per module, the way the arm's own feature test builds it (the CPU oracle on the
masked / reduced / anchored records), and does not depend on the launch shape; a case is then one engine run.  Bit-exact
(integer work).  The fixture also checks, without a GPU, that no comparison is vacuous and that under `two_wg_overflow`
every tile holds a record that overflows the staged prefix."""
import struct
from dataclasses import dataclass, field

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import end_condition_lib as ec
import gapped_lib as gl
import pssbam_testlib as tl
import regions_lib as rl
import site_context_lib as sc
from test_gpu_contig_sets import oracle_sets
from test_gpu_kmer_planes import fk_dict, oracle_on_contigs
from test_gpu_length_bins import bins_of, oracle_bins
from test_gpu_length_hist import CLASSES, flag_class, oracle_ok_rows
from test_gpu_read_groups import first_rg

pytestmark = pytest.mark.gpu

N_READS = 3200      # 67 tiles of 48: >= 64 as the XCD mapping requires, no multiple of 8 (the last XCD's share is short); 50 tiles of 64
OVERFLOW_PIECES = 5  # 16-byte pieces staged per record under `two_wg_overflow`

# environment of the engine -> launch shape of the tiled family
SHAPES = {
    "one_wg": {"PSSBAM_GRID_WGS": "1", "PSSBAM_TILE_READS": "48"},
    "three_wg": {"PSSBAM_GRID_WGS": "3", "PSSBAM_TILE_READS": "48"},
    "two_wg_overflow": {"PSSBAM_GRID_WGS": "2", "PSSBAM_TILE_READS": "64", "PSSBAM_PIECES": str(OVERFLOW_PIECES)},
    "xcd8": {"PSSBAM_XCD_MAP": "1", "PSSBAM_GRID_WGS": "8", "PSSBAM_TILE_READS": "48"},
    "xcd16": {"PSSBAM_XCD_MAP": "1", "PSSBAM_GRID_WGS": "16", "PSSBAM_TILE_READS": "48"},
}
NO_XCD = ["one_wg", "three_wg", "two_wg_overflow"]     # tally_compact ignores xcd_map
SIMPLE_SHAPE = {"PSSBAM_SIMPLE_BLOCKS": "1"}           # 3 200 records in 256 lanes: 13 trips of the stride loop

HIST_MAX = 100
END_COND = (2, *ec.PRESETS["ds"])
LEN_EDGES = {25: [35, 50, 75], 40: [50, 65, 90]}       # -S by -r: 3 edges, 4 bins none of which lies below -r (and the empty plane 0)
KMER_EDGES = [30, 60]
CONTIG_SETS = {"big": ["chrB", "chrMissing"], "chrA": ["chrA"], "small": ["tiny.4", "nowhere"]}   # scaffold_10 stays in plane 0
RG_IDS = ["grpA", "grpB"]
GAPPED_TILED_OPS = 16                                  # CIGAR ops a lane of the tiled kernel walks (pss_bam_amd.GAPPED_TILED_OPS)


# ---- datasets and expectations (CPU only) ---------------------------------------------------------------------------

@dataclass
class Data:
    contigs: list
    refs: list
    recs: list
    raw: np.ndarray = None
    loaded: list = None

    def __post_init__(self):
        self.raw = tl.raw_records(self.refs, self.recs)
        self.loaded = tl.loaded_contigs(self.contigs)


@dataclass
class Arm:
    data: str                       # key of the dataset
    kw: dict                        # Engine keyword arguments (kernel excepted)
    want: dict                      # the expectation, see check()
    env: dict = field(default_factory=dict)    # environment beside the shape's
    regions: list = None            # -T intervals
    min_slow: int = 0               # records that take the one-lane path under every shape


def needed_prefixes(raw: np.ndarray) -> list:
    """[(offset, qual_off + 1)] of every record of a BAM record block: the prefix the tallies read (the engine stages
    more, never less, where -R / -G / -Q walk further into the record)"""
    b, o, out = raw.tobytes(), 0, []
    while o < len(b):
        bs, = struct.unpack_from("<I", b, o)
        n_cig, = struct.unpack_from("<H", b, o + 16)
        l_seq, = struct.unpack_from("<I", b, o + 20)
        out.append((o, 36 + b[o + 12] + 4 * n_cig + (l_seq + 1) // 2 + 1))
        o += 4 + bs
    return out


def assert_every_tile_overflows(raw: np.ndarray, tile: int = 64, pieces: int = OVERFLOW_PIECES):
    """A record is staged from its 16-byte aligned address, so pieces * 16 - (offset & 15) of its bytes are in LDS: more than
    pieces * 16 - 15 whatever the offset.  Every tile must hold a record that needs more than it has."""
    need = needed_prefixes(raw)
    assert len(need) == N_READS
    for t in range(0, len(need), tile):
        assert any(n > pieces * 16 - (o & 15) for o, n in need[t:t + tile]), f"no overflow record in tile {t // tile}"


def stats_of(n_records: int, st, kst=None, pss: bool = True, **more) -> dict:
    """the status counters an engine must report, from the oracle's of the pss run (and of the fragkon run)"""
    out = {"records": n_records, "parse_skip": int(st[tl.ST_PARSE_SKIP]), "no_contig": int(st[tl.ST_NO_CONTIG]), **more}
    if pss:
        out.update(pss_ok=int(st[tl.ST_OK]), pss_filtered=int(st[tl.ST_FILTERED]))
    if kst is not None:
        out.update(kmer_ok=int(kst[tl.ST_OK]), kmer_filtered=int(kst[tl.ST_FILTERED]), kmer_fail=int(kst[tl.ST_KMER_FAIL]))
    return out


def region_stats(n_records: int, plain, red, kplain=None, kred=None, **more) -> dict:
    """the counters of a run with -T from the oracle's on the unreduced (plain) and the reduced input: RECORDS, PARSE_SKIP
    and NO_CONTIG as without regions; a candidate that meets no region is FILTERED"""
    out = stats_of(n_records, plain, **more)
    out.update(pss_ok=int(red[tl.ST_OK]), pss_filtered=int(plain[tl.ST_FILTERED] + plain[tl.ST_OK] - red[tl.ST_OK]))
    if kplain is not None:
        done = lambda st: int(st[tl.ST_OK] + st[tl.ST_KMER_FAIL])   # noqa: E731
        out.update(kmer_ok=int(kred[tl.ST_OK]), kmer_fail=int(kred[tl.ST_KMER_FAIL]),
                   kmer_filtered=int(kplain[tl.ST_FILTERED]) + done(kplain) - done(kred))
    return out


def direct_hist(contigs, recs, o: tl.PssOpts, m: int) -> dict:
    """{flag class: (hf, hr)}: the length (|TLEN| when paired, else strlen(SEQ)) of every read that site_context_lib's
    direct count adds to the forward / reverse table, lengths above m in row m + 1"""
    out = {c: (np.zeros(m + 2, dtype=np.uint64), np.zeros(m + 2, dtype=np.uint64)) for c in CLASSES}
    for r in recs:
        f, rv = sc.direct_counts(contigs, [r], o, None)
        row = min(abs(r.tlen) if r.flag & 1 else len(r.seq), m + 1)
        out[flag_class(r)][0][row] += int(f.any())
        out[flag_class(r)][1][row] += int(rv.any())
    return out


def one_lane_gapped(contigs, recs, o: tl.PssOpts) -> tuple:
    """(long, near): the -I records the tiled kernel hands to its one-lane path under every shape and that are tallied there
    -- those with more CIGAR ops than a lane walks, and among the others those with a gap whose far run begins within
    region_len reference bases of an end"""
    n_long = n_near = 0
    for r in recs:
        an = gl.anchor_info(r)
        if an is None:
            continue
        span, a, b = an["span"], an["a"], an["b"]
        long_cigar = len(r.cigar) > GAPPED_TILED_OPS
        if long_cigar or (a != span and (span - b < o.region_len or span - a < o.region_len)):
            f, rv = gl.direct_counts(contigs, [r], o)
            n_long += int(long_cigar and (f.any() or rv.any()))
            n_near += int(not long_cigar and (f.any() or rv.any()))
    return n_long, n_near


def sam_of(tmp, name, refs, recs):
    p = tmp / name
    tl.write_sam(p, refs, recs)
    return p


def build_arms(oracle, tmp):
    """-> (datasets, arms): every dataset, every arm's Engine arguments and expectation, and the checks that no
    comparison is vacuous.  Nothing here touches a GPU."""
    D, A = {}, {}
    D["plain"] = Data(*tl.fuzz_dataset(9601, N_READS))
    D["sets"] = Data(*tl.fuzz_dataset(9602, N_READS, contig_lens=(5000, 1200, 300, 900)))
    D["rg"] = Data(*tl.fuzz_dataset(9603, N_READS, with_rg=True))
    c, f, r = tl.fuzz_dataset(9604, N_READS)
    D["dmg"] = Data(c, f, ec.plant_damage(c, r, np.random.default_rng(9605), 0.5))
    D["gap"] = Data(*gl.fuzz_case(9606, N_READS)[:3])
    for d in D.values():
        assert len(d.recs) == N_READS
        assert_every_tile_overflows(d.raw)

    def table_pair(t):
        assert t[0][2:].any() and t[1][2:].any() and t[0][:2].any() and t[1][:2].any()
        return t[0], t[1]

    def kmer_pair(k5, k3):
        assert k5.any() and k3.any()
        return k5, k3

    # ---- the plain dataset: tally_compact, -Q, -T, -H, -X, -S, the lane-per-read cross-check --------------------------
    p = D["plain"]
    g = oracle.genome_from_arrays(p.loaded)
    sam = sam_of(tmp, "plain.sam", p.refs, p.recs)
    kst = {}
    kmer = {}
    for k in (4, 5, 9):
        k5, k3, kst[k] = oracle.fragkon(g, sam, tl.FkOpts(klen=k))
        kmer[k] = kmer_pair(k5, k3)
    plain = {}
    for n in (7, 15, 16, 25, 40):
        wf, wr, st = oracle.pss(g, sam, tl.PssOpts(region_len=n))
        plain[n] = (table_pair((wf, wr)), st)
    # 1. tally_compact (-r <= 16): alone, with k-mers in LDS (k = 4) and with global k-mer bins (k = 9)
    for n in (7, 15, 16):
        for k in (None, 4, 9):
            A[f"compact_r{n}" + (f"_k{k}" if k else "")] = Arm(
                "plain", dict(pss=dict(region_len=n), kmer=dict(klen=k) if k else None),
                dict(tables=plain[n][0], kmer=kmer[k] if k else None, stats=stats_of(N_READS, plain[n][1], kst[k] if k else None)))
    for name in ("compact_r15", "compact_r15_k4"):
        A[name.replace("compact", "plan_once")] = Arm("plain", A[name].kw, A[name].want, env={"PSSBAM_COMPACT_PLAN_ONCE": "1"})
    # 2. -Q 20: QUAL is read from the staging buffer (-r 40: again in the second row pass)
    masked = sam_of(tmp, "q20.sam", p.refs, bq.mask_recs(p.recs, 20))
    for n in (25, 40):
        wf, wr, st = oracle.pss(g, masked, tl.PssOpts(region_len=n))
        assert (wf[2:] != plain[n][0][0][2:]).any() and (wr[2:] != plain[n][0][1][2:]).any()      # the mask bites
        A[f"Q20_r{n}"] = Arm("plain", dict(pss=dict(region_len=n), min_base_qual=20), dict(tables=table_pair((wf, wr)), stats=stats_of(N_READS, st)))
    # 3. -T: -r 15 goes to tally_tiled because of the regions
    ivs = rl.fuzz_intervals(9601, p.contigs, p.recs)
    red = sam_of(tmp, "red.sam", p.refs, rl.reduce_recs(p.recs, ivs))
    k5, k3, kred = oracle.fragkon(g, red, tl.FkOpts(klen=4))
    assert 0 < kred[tl.ST_OK] < kst[4][tl.ST_OK]
    for n, k in ((15, None), (40, None), (40, 4)):
        wf, wr, st = oracle.pss(g, red, tl.PssOpts(region_len=n))
        assert 0 < st[tl.ST_OK] < plain[n][1][tl.ST_OK]
        A[f"T_r{n}" + ("_k4" if k else "")] = Arm(
            "plain", dict(pss=dict(region_len=n), kmer=dict(klen=4) if k else None),
            dict(tables=table_pair((wf, wr)), kmer=kmer_pair(k5, k3) if k else None,
                 stats=region_stats(N_READS, plain[n][1], st, kst[4] if k else None, kred if k else None)), regions=ivs)
    # 4. -H 100: the two LDS histograms are accumulated over the loop; reads longer than 100 share the last bin
    o = tl.PssOpts(region_len=25)
    by_class = direct_hist(p.contigs, p.recs, o, HIST_MAX)
    zero = np.zeros(HIST_MAX + 2, dtype=np.uint64)
    for c in CLASSES:           # the direct count against the oracle, row by row: its PSS_OK with -l x -L x on each flag class
        rows = oracle_ok_rows(oracle, g, sam_of(tmp, f"h_{c}.sam", p.refs, [r for r in p.recs if flag_class(r) == c]), o, HIST_MAX)
        hf, hr = by_class[c]
        want = {"unpaired": (rows, rows), "first": (rows, zero), "second": (zero, rows)}.get(c)
        assert (np.array_equal(hf, want[0]) and np.array_equal(hr, want[1])) if want else np.array_equal(hf + hr, rows), c
    hf, hr = sum(v[0] for v in by_class.values()), sum(v[1] for v in by_class.values())
    assert hf[25:101].sum() > 100 and hr[25:101].sum() > 100 and hf[101] > 0 and hr[101] > 0 and not np.array_equal(hf, hr)
    A["H100_r25"] = Arm("plain", dict(pss=dict(region_len=25), length_hist=HIST_MAX), dict(tables=plain[25][0], hist=(hf, hr), stats=stats_of(N_READS, plain[25][1])))
    # 5. -X cpg: a second LDS table over the loop
    site_sams = {keep: sam_of(tmp, f"site{int(keep)}.sam", p.refs, sc.mask_recs(p.contigs, p.recs, keep)) for keep in (True, False)}
    for n in (25, 40):
        o = tl.PssOpts(region_len=n)
        w_in, w_out = table_pair(oracle.pss(g, site_sams[True], o)[:2]), table_pair(oracle.pss(g, site_sams[False], o)[:2])
        A[f"X_r{n}"] = Arm("plain", dict(pss=dict(region_len=n), site_context="cpg"), dict(tables=plain[n][0], site=(w_in, w_out), stats=stats_of(N_READS, plain[n][1])))
    # 8a. -S: planes of the substitution tables
    for n in (25, 40):
        o = tl.PssOpts(region_len=n)
        bins = {key: table_pair(t) for key, t in oracle_bins(oracle, g, sam, o, LEN_EDGES[n]).items()}
        assert list(bins) == bins_of(o, LEN_EDGES[n])
        A[f"S_r{n}"] = Arm("plain", dict(pss=dict(region_len=n), length_bins=LEN_EDGES[n]), dict(tables=plain[n][0], planes=("bins", bins), stats=stats_of(N_READS, plain[n][1])))
    # 9a. k-mer planes by read length: LDS bins at k = 4, global bins at k = 6
    for k in (4, 6):
        fo = tl.FkOpts(klen=k)
        k5, k3, st = oracle.fragkon(g, sam, fo)
        bins = {}
        for lo, hi in bins_of(fo, KMER_EDGES):
            b5, b3, _ = oracle.fragkon(g, sam, tl.FkOpts(klen=k, min_read_len=lo, max_read_len=hi))
            bins[(lo, hi)] = kmer_pair(b5, b3)
        A[f"kS_k{k}"] = Arm("plain", dict(kmer=fk_dict(fo), length_bins=KMER_EDGES), dict(kmer=kmer_pair(k5, k3), planes=("bins", bins), stats=stats_of(N_READS, st, st, pss=False)))
    # 11a. the lane-per-read kernel's own plain case
    A["plain_r25_k5"] = Arm("plain", dict(pss=dict(region_len=25), kmer=dict(klen=5)), dict(tables=plain[25][0], kmer=kmer[5], stats=stats_of(N_READS, plain[25][1], kst[5])))
    oracle.free_genome(g)

    # ---- -C: four contigs, three sets, scaffold_10 unassigned ---------------------------------------------------------
    s = D["sets"]
    g = oracle.genome_from_arrays(s.loaded)
    sam = sam_of(tmp, "sets.sam", s.refs, s.recs)
    for n in (25, 40):
        o = tl.PssOpts(region_len=n)
        wf, wr, st = oracle.pss(g, sam, o)
        sets = {key: table_pair(t) for key, t in oracle_sets(oracle, s.contigs, sam, o, CONTIG_SETS).items()}
        assert (wf - sum(t[0] for t in sets.values()))[2:].any()                                # plane 0 is not empty
        A[f"C_r{n}"] = Arm("sets", dict(pss=dict(region_len=n), contig_sets=CONTIG_SETS), dict(tables=table_pair((wf, wr)), planes=("sets", sets), stats=stats_of(N_READS, st)))
    for k in (4, 6):
        fo = tl.FkOpts(klen=k)
        k5, k3, st = oracle.fragkon(g, sam, fo)
        sets = {label: kmer_pair(*oracle_on_contigs(oracle, s.contigs, names, sam, fo)) for label, names in CONTIG_SETS.items()}
        A[f"kC_k{k}"] = Arm("sets", dict(kmer=fk_dict(fo), contig_sets=CONTIG_SETS), dict(kmer=kmer_pair(k5, k3), planes=("sets", sets), stats=stats_of(N_READS, st, st, pss=False)))
    oracle.free_genome(g)

    # ---- read groups: k-mer planes by @RG, and -R -Q -T together (whole records staged, all three filters) ------------
    q = D["rg"]
    g = oracle.genome_from_arrays(q.loaded)
    sam = sam_of(tmp, "rg.sam", q.refs, q.recs)
    for k in (4, 6):
        fo = tl.FkOpts(klen=k)
        k5, k3, st = oracle.fragkon(g, sam, fo)
        groups = {}
        for key in [None] + RG_IDS:
            sel = [r for r in q.recs if (first_rg(r) == key if key is not None else first_rg(r) not in RG_IDS)]
            g5, g3, _ = oracle.fragkon(g, sam_of(tmp, "grp.sam", q.refs, sel), fo)
            groups[key] = kmer_pair(g5, g3)
        A[f"kG_k{k}"] = Arm("rg", dict(kmer=fk_dict(fo), read_groups=RG_IDS), dict(kmer=kmer_pair(k5, k3), planes=("groups", groups), stats=stats_of(N_READS, st, st, pss=False)))
    o = tl.PssOpts(region_len=25)
    keep = [r for r in q.recs if first_rg(r) == "grpA"]
    ivs = rl.fuzz_intervals(9603, q.contigs, q.recs)
    kept = rl.reduce_recs(keep, ivs)
    _, _, st_keep = oracle.pss(g, sam_of(tmp, "keep.sam", q.refs, keep), o)
    wf, wr, st = oracle.pss(g, sam_of(tmp, "keep_red_q20.sam", q.refs, bq.mask_recs(kept, 20)), o)
    uf, _, _ = oracle.pss(g, sam_of(tmp, "keep_red.sam", q.refs, kept), o)
    assert 0 < st[tl.ST_OK] < st_keep[tl.ST_OK] and (uf[2:] != wf[2:]).any() and 0 < len(keep) < N_READS
    A["R_Q20_T_r25"] = Arm("rg", dict(pss=dict(region_len=25), read_group="grpA", min_base_qual=20),
                           dict(tables=table_pair((wf, wr)), stats=region_stats(N_READS, st_keep, st, rg_dropped=N_READS - len(keep))), regions=ivs)
    oracle.free_genome(g)

    # ---- -E ds,2 on planted damage ------------------------------------------------------------------------------------
    d = D["dmg"]
    g = oracle.genome_from_arrays(d.loaded)
    o = tl.PssOpts(region_len=25)
    wf, wr, st = oracle.pss(g, sam_of(tmp, "dmg.sam", d.refs, d.recs), o)
    cf, cr, reads = ec.expected(oracle, g, tmp, d.refs, d.contigs, d.recs, o, *END_COND)
    assert cf[2:].any() and cr[2:].any() and reads[0] > reads[1] >= 20 and reads[0] > reads[2] >= 20 and reads[3] >= 5
    A["E_ds2_r25"] = Arm("dmg", dict(pss=dict(region_len=25), end_condition=END_COND), dict(tables=table_pair((wf, wr)), end=(cf, cr, reads), stats=stats_of(N_READS, st)))
    oracle.free_genome(g)

    # ---- -I: the CIGAR walk in the staging buffer; long CIGARs and gaps near an end on the one-lane path ----------------
    a = D["gap"]
    g = oracle.genome_from_arrays(a.loaded)
    anchored = sam_of(tmp, "anchored.sam", a.refs, gl.anchor_recs(a.recs))
    as_is = sam_of(tmp, "gap.sam", a.refs, a.recs)
    for n in (25, 40):
        o = tl.PssOpts(region_len=n)
        wf, wr, st = oracle.pss(g, anchored, o)
        assert st[tl.ST_OK] > oracle.pss(g, as_is, o)[2][tl.ST_OK] + 200
        n_long, n_near = one_lane_gapped(a.contigs, a.recs, o)
        assert n_long >= 20 and n_near >= 20
        A[f"I_r{n}"] = Arm("gap", dict(pss=dict(region_len=n), gapped=True), dict(tables=table_pair((wf, wr)), stats=stats_of(N_READS, st)), min_slow=n_long + n_near)
    oracle.free_genome(g)
    return D, A


# ---- the cases ------------------------------------------------------------------------------------------------------

COMPACT = [f"compact_r{n}{k}" for n in (7, 16) for k in ("", "_k4", "_k9")] + ["plan_once_r15", "plan_once_r15_k4"]
TILED = ["Q20_r25", "Q20_r40", "T_r15", "T_r40", "T_r40_k4", "H100_r25", "X_r25", "X_r40", "E_ds2_r25", "I_r25", "I_r40",
         "S_r25", "S_r40", "C_r25", "C_r40", "kS_k4", "kS_k6", "kG_k4", "kG_k6", "kC_k4", "kC_k6", "R_Q20_T_r25"]
SIMPLE = ["plain_r25_k5", "Q20_r25", "T_r15", "H100_r25", "X_r25", "E_ds2_r25", "I_r25", "S_r25", "kS_k4"]
FEED = ["compact_r15", "Q20_r25"]
ALL_ARMS = set(COMPACT + TILED + SIMPLE + FEED)


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


@pytest.fixture(scope="module")
def built(oracle, tmp_path_factory):
    D, A = build_arms(oracle, tmp_path_factory.mktemp("tile_loop"))
    assert ALL_ARMS <= set(A)
    return D, A


def same(got, want):
    return np.array_equal(got, np.asarray(want).astype(np.uint64))


def check(eng, want: dict):
    """every table the arm exposes and its status counters against the expectation; -> the totals"""
    if "hist" in want:
        hf, hr = eng.finish_length_hist()
        assert same(hf, want["hist"][0]) and same(hr, want["hist"][1]), "length histograms differ"
    fin = eng.finish_site_context() if "site" in want else None
    if "end" in want:
        got = eng.finish_end_condition()
        for k, name in enumerate(("COND.fwd", "COND.rev", "reads")):
            assert same(got[k], want["end"][k]), (name, got[2], want["end"][2])
    if "planes" in want:
        kind, exp = want["planes"]
        got = {"bins": eng.finish_bins, "sets": eng.finish_sets, "groups": eng.finish_groups}[kind]()
        assert set(got) == set(exp)
        for key, (a, b) in exp.items():
            t = got[key]
            assert (same(t.k5, a) and same(t.k3, b)) if t.fwd is None else (same(t.fwd, a) and same(t.rev, b)), (kind, key)
    if "mism" in want:
        mf, mr = eng.finish_mismatches()
        assert same(mf, want["mism"][0]) and same(mr, want["mism"][1]), "mismatch histograms differ"
    if "contigs" in want:
        got = eng.finish_contigs()
        assert sorted(got) == sorted(want["contigs"])
        for k, (wf, wr) in want["contigs"].items():
            assert same(got[k].fwd, wf) and same(got[k].rev, wr), ("contig plane", k)
    if "replicates" in want:
        fwd, rev = eng.finish_replicates()
        assert len(fwd) == len(rev) == len(want["replicates"])
        for j, (wf, wr) in enumerate(want["replicates"]):
            assert same(fwd[j], wf) and same(rev[j], wr), ("replicate", j)
    if "interior" in want:
        table, reads = eng.finish_interior()
        assert same(table, want["interior"][0]) and reads == want["interior"][1], ("interior table differs", reads, want["interior"][1])
    if "composition" in want:
        c5, c3 = eng.finish_composition()
        assert same(c5, want["composition"][0]) and same(c3, want["composition"][1]), "composition blocks differ"
    tot = eng.finish()
    if want.get("tables") is not None:
        assert same(tot.fwd, want["tables"][0]) and same(tot.rev, want["tables"][1]), "substitution tables differ"
    if want.get("kmer") is not None:
        assert same(tot.k5, want["kmer"][0]) and same(tot.k3, want["kmer"][1]), "k-mer tables differ"
    if fin is not None:
        (in_f, in_r), (out_f, out_r) = want["site"]
        for t, got, w_in, w_out in ((tot.fwd, fin[0], in_f, out_f), (tot.rev, fin[1], in_r, out_r)):
            assert same(got, w_in) and same(t[2:] - got[2:], w_out[2:]) and same(got[:2], t[:2]), "in-context tables differ"
    assert {k: tot.stats[k] for k in want["stats"]} == want["stats"]
    return tot


def run_arm(pkg, built, name: str, kernel: int, feed=None):
    D, A = built
    arm, d = A[name], D[A[name].data]
    eng = pkg.Engine(kernel=kernel, **arm.kw)
    try:
        if feed is not None:
            eng.feed_open(len(d.refs))
            eng.submit_bgzf(feed[0], header_bytes=feed[1], max_batch_inflated=70000)
        if arm.regions is not None:
            eng.set_regions(*rl.to_arrays(arm.regions))
        eng.set_genome_arrays(d.loaded)
        eng.set_references([nm for nm, _ in d.refs])
        if feed is None:
            eng.submit(d.raw)
        tot = check(eng, arm.want)
        if feed is not None:
            assert eng.feed_status()["flags"] == 0
        return tot, arm
    finally:
        eng.close()


def set_env(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


def tiled_case(pkg, built, monkeypatch, name, shape, extra=None):
    set_env(monkeypatch, SHAPES[shape], built[1][name].env, extra or {})
    tot, arm = run_arm(pkg, built, name, pkg.KERNEL_AUTO)
    assert tot.stats["slow_path"] >= arm.min_slow
    if shape == "two_wg_overflow":      # (every tile holds an overflow record: assert_every_tile_overflows)
        assert tot.stats["slow_path"] >= 50


@pytest.mark.parametrize("shape", NO_XCD)
@pytest.mark.parametrize("name", COMPACT)
def test_compact_walks_several_tiles(pkg, built, monkeypatch, name, shape):
    """tally_compact and its PLAN_ONCE form; under `two_wg_overflow` the overflow queue is refilled and reset every tile"""
    tiled_case(pkg, built, monkeypatch, name, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", TILED)
def test_tiled_arms_walk_several_tiles(pkg, built, monkeypatch, name, shape):
    """tally_tiled's option arms, tally_tiled_planes and tally_tiled_kmer_planes, with and without the XCD mapping"""
    tiled_case(pkg, built, monkeypatch, name, shape)


@pytest.mark.parametrize("name", ["S_r40", "C_r40"])
def test_plane_passes_by_row_passes_by_tiles(pkg, built, monkeypatch, name):
    """two plane slots per launch: plane passes x row passes, one workgroup walking every tile in each"""
    tiled_case(pkg, built, monkeypatch, name, "one_wg", {"PSSBAM_GROUP_SLOTS": "2"})


@pytest.mark.parametrize("name", SIMPLE)
def test_lane_per_read_kernels_take_several_records(pkg, built, monkeypatch, name):
    """tally_simple, tally_simple_planes and tally_simple_kmer_planes in one block: every thread takes 12 or 13 records"""
    set_env(monkeypatch, SIMPLE_SHAPE)
    run_arm(pkg, built, name, pkg.KERNEL_SIMPLE)


@pytest.fixture(scope="module")
def bam_feed(built, tmp_path_factory):
    """the plain dataset as a BGZF BAM in 300-byte blocks: records (and their length words) cross blocks"""
    d = built[0]["plain"]
    bam = tmp_path_factory.mktemp("tile_loop_feed") / "x.bam"
    tl.write_bam(bam, d.refs, d.recs, block=300)
    return np.frombuffer(bam.read_bytes(), dtype=np.uint8), len(tl.bam_bytes(d.refs, []))


@pytest.mark.parametrize("shape", ["three_wg", "two_wg_overflow"])
@pytest.mark.parametrize("name", FEED)
def test_compressed_feed_with_a_small_grid(pkg, built, bam_feed, monkeypatch, name, shape):
    """device-indexed blocks: the launch geometry comes from an upper bound on the record count, the count from device memory"""
    set_env(monkeypatch, SHAPES[shape])
    tot, _ = run_arm(pkg, built, name, pkg.KERNEL_AUTO, feed=bam_feed)
    if shape == "two_wg_overflow":
        assert tot.stats["slow_path"] > 0

"""The record sink (pssbam_engine_set_record_sink, pss-bam -O) on the GPU: the records the engine hands over are exactly the
ones it added to a table -- byte-identical, in input order -- under every filter, on every submit path, at every size the
selection's scan and gather change their path at.

Nothing on the expected side comes from the engine.  For a record set R and an option set X:
  1. the kept bytes split into records that are a subsequence of R, byte for byte and in order;
  2. their number is PSS_OK of the CPU oracle on R under X;
  3. the oracle on the kept records under X gives the tables it gives on R;
  4. the oracle on the dropped records under X gives all-zero tables and PSS_OK == 0;
  5. the engine's own tables and status counters are those of the run without a sink.
"Under X" for the options the oracle has no switch for is the restatement of that option's own yardstick (regions_lib,
gapped_lib, mismatch_lib, read_score_lib, base_quality_lib): the oracle on the reduced / rewritten records."""
import ctypes as C
import struct
from dataclasses import dataclass, replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import gapped_lib as gl
import mismatch_lib as ml
import pssbam_testlib as tl
import read_score_lib as rs
import regions_lib as rl

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
SCAN_TILE = 1024          # csrc/select_kernels.h SELECT_SCAN_TILE: entries of len[] per workgroup of the scan
SUMS_ROUND = 256          # ... SELECT_SUMS_ROUND: tile sums per round of the scan's second level
# pssbam_engine_kernel_time's launch count for LAUNCH_INPUT without a sink, taken from the commit before the sink existed
LAUNCH_INPUT = (7, 3000)  # tl.fuzz_dataset(seed, n_reads), one submit, pss region_len 15
LAUNCHES_BEFORE_THE_SINK = 1


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


# ---- record sets ------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    contigs: list      # [(id, text)]
    refs: list         # [(name, len)]
    recs: list         # tl.Rec, in the order of raw
    raw: np.ndarray    # the BAM records
    ivs: list          # -T intervals [(name, start, end)]


def split_records(raw: np.ndarray) -> list:
    out, o = [], 0
    b = raw.tobytes()
    while o < len(b):
        n = 4 + struct.unpack_from("<I", b, o)[0]
        assert o + n <= len(b), "record set ends inside a record"
        out.append(b[o:o + n])
        o += n
    return out


def parse_bed(path: Path) -> list:
    ivs = []
    for ln in path.read_text().splitlines():
        f = ln.split()
        if len(f) >= 3 and f[1].isdigit() and f[2].isdigit() and f[0] not in ("track", "browser"):
            ivs.append((f[0], int(f[1]), int(f[2])))
    return ivs


def golden_case(base: str) -> Case:
    fa_txt = (GOLD / f"{base}.fa").read_text()
    contigs = [(blk.split("\n", 1)[0].split()[0], "".join(blk.split("\n")[1:])) for blk in fa_txt.split(">")[1:]]
    refs, raw = tl.read_bam(GOLD / f"{base}.bam")
    _, recs = ml.read_sam(GOLD / f"{base}.sam")
    lines = [ln for ln in (GOLD / f"{base}.sam").read_text().splitlines() if not ln.startswith("@")]
    recs = [replace(r, tags=[("RG", "Z", f[5:]) for f in ln.split("\t")[11:] if f.startswith("RG:Z:")]) for r, ln in zip(recs, lines)]
    blobs = split_records(raw)
    assert len(blobs) == len(recs) and all(b[36:36 + b[12] - 1].decode() == r.qname for b, r in zip(blobs, recs))
    ivs = parse_bed(GOLD / "regions_setA.bed") if base == "setA" else [(nm, ln // 4, ln // 2) for nm, ln in refs]
    return Case(contigs, refs, recs, raw, ivs)


def fuzz_case(seed: int) -> Case:
    contigs, refs, recs = tl.fuzz_dataset(seed, 1500, with_rg=True)
    return Case(contigs, refs, recs, tl.raw_records(refs, recs), rl.fuzz_intervals(seed, contigs, recs))


_CASES: dict = {}


def case_of(name: str) -> Case:
    if name not in _CASES:
        _CASES[name] = golden_case(name) if name.startswith("set") else fuzz_case(int(name[4:]))
    return _CASES[name]


# ---- option sets: (PssOpts, what to set on the engine, the restatement on records) --------------------------------------------

W_PMD = rs.committed_pmd_weights()


@dataclass
class Opt:
    o: tl.PssOpts
    setup: object = None          # f(eng, case)
    reduce: object = None         # f(recs, case) -> the records the plain oracle takes
    rg: str = None
    cli: tuple = ()


def _set_regions(eng, c):
    eng.set_regions(*rl.to_arrays(c.ivs))


OPTS = {
    "none": Opt(tl.PssOpts()),
    "q30": Opt(tl.PssOpts(min_mq=30)),
    "l40_L60": Opt(tl.PssOpts(min_read_len=40, max_read_len=60)),
    "m": Opt(tl.PssOpts(merged_only=True)),
    "U_A_D_GT": Opt(tl.PssOpts(up_ctx="A", down_ctx="GT")),
    "R": Opt(tl.PssOpts(), rg="grpA", reduce=lambda recs, c: [r for r in recs if ("RG", "Z", "grpA") in r.tags]),
    "T": Opt(tl.PssOpts(), setup=_set_regions, reduce=lambda recs, c: rl.reduce_recs(recs, c.ivs)),
    "I": Opt(tl.PssOpts(), setup=lambda e, c: e.set_gapped(True), reduce=lambda recs, c: gl.anchor_recs(recs)),
    "n1": Opt(tl.PssOpts(), setup=lambda e, c: e.set_mismatches(0, 1, 0), reduce=lambda recs, c: ml.reduce_to(recs, c.contigs, 1)),
    "n0_V": Opt(tl.PssOpts(), setup=lambda e, c: e.set_mismatches(0, 0, 1), reduce=lambda recs, c: ml.reduce_to(recs, c.contigs, 0, tv_only=True)),
    "y3": Opt(tl.PssOpts(), setup=lambda e, c: e.set_read_score(W_PMD, 768), reduce=lambda recs, c: rs.reduce_to(recs, c.contigs, W_PMD, 768)),
    "y3_Q20": Opt(tl.PssOpts(), setup=lambda e, c: (e.set_min_base_quality(20), e.set_read_score(W_PMD, 768)),
                  reduce=lambda recs, c: bq.mask_recs(rs.reduce_to(recs, c.contigs, W_PMD, 768, 20), 20)),
    "q20_G": Opt(tl.PssOpts(min_mq=20), setup=lambda e, c: e.set_read_groups(["grpA", "grpB"])),
}
# the committed tables of the reference on the reduced inputs: (option set, record set) -> golden
GOLDENS = {("y3", "setD"): "pmd3_setD", ("n1", "setA"): "mism1_setA", ("n0_V", "setD"): "mismtv0_setD", ("T", "setA"): "regions_setA"}


def pss_dict(o: tl.PssOpts):
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq,
                up_ctx=o.up_ctx, down_ctx=o.down_ctx, merged_only=o.merged_only)


def make_engine(pkg, c: Case, x: Opt, sink=True, kernel=0):
    eng = pkg.Engine(pss=pss_dict(x.o), read_group=x.rg, kernel=kernel)
    if x.setup:
        x.setup(eng, c)
    if sink:
        eng.set_record_sink()
    eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
    eng.set_references([n for n, _ in c.refs])
    return eng


def run(pkg, c: Case, x: Opt, sink=True, raw=None, chunks=1, kernel=0):
    """-> (Tables, kept bytes or None, records the sink reported)"""
    raw = c.raw if raw is None else raw
    eng = make_engine(pkg, c, x, sink, kernel)
    try:
        offs = pkg.index_records(raw)
        n = offs.size - 1
        cuts = [n * i // chunks for i in range(chunks + 1)]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if b > a:
                o = offs[a:b + 1].astype(np.int64)
                eng.submit(raw[o[0]:o[-1]], (o - o[0]).astype(np.uint32))
        kept = eng.finish_records() if sink else None
        return eng.finish(), kept, getattr(eng, "records_kept", 0)
    finally:
        eng.close()


def kept_indices(all_blobs: list, kept: np.ndarray) -> list:
    """check 1: the kept bytes are whole records, each byte-identical to a record of the input, in the input's order"""
    idx, j = [], 0
    for b in split_records(kept):
        while j < len(all_blobs) and all_blobs[j] != b:
            j += 1
        assert j < len(all_blobs), "a delivered record is not in the input, or out of order"
        idx.append(j)
        j += 1
    return idx


def oracle_on(oracle, g, tmp_path, c: Case, x: Opt, recs: list):
    sam = tmp_path / "x.sam"
    tl.write_sam(sam, c.refs, x.reduce(recs, c) if x.reduce else recs)
    return oracle.pss(g, sam, x.o)


@pytest.mark.parametrize("xname", list(OPTS))
@pytest.mark.parametrize("cname", ["setA", "setD", "fuzz4401"])
def test_kept_records_are_the_tallied_ones(pkg, oracle, tmp_path, cname, xname):
    c, x = case_of(cname), OPTS[xname]
    tabs, kept, n_reported = run(pkg, c, x)
    blobs = split_records(c.raw)
    idx = kept_indices(blobs, kept)                                                          # 1
    assert n_reported == len(idx)
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, c.contigs)
    g = oracle.load_genome(fa)
    try:
        wf, wr, wst = oracle_on(oracle, g, tmp_path, c, x, c.recs)
        assert len(idx) == int(wst[tl.ST_OK])                                                # 2
        kf, kr, kst = oracle_on(oracle, g, tmp_path, c, x, [c.recs[i] for i in idx])
        assert np.array_equal(kf, wf) and np.array_equal(kr, wr) and int(kst[tl.ST_OK]) == len(idx)   # 3
        gone = sorted(set(range(len(blobs))) - set(idx))
        df, dr, dst = oracle_on(oracle, g, tmp_path, c, x, [c.recs[i] for i in gone])
        assert not df.any() and not dr.any() and int(dst[tl.ST_OK]) == 0                     # 4
    finally:
        oracle.free_genome(g)
    plain, _, _ = run(pkg, c, x, sink=False)
    assert np.array_equal(tabs.fwd, plain.fwd) and np.array_equal(tabs.rev, plain.rev) and tabs.stats == plain.stats   # 5
    assert np.array_equal(tabs.fwd, wf) and np.array_equal(tabs.rev, wr)
    if cname == "fuzz4401" and xname != "R":
        assert 0 < len(idx) < len(blobs)            # (not vacuous: something kept, something dropped)
    if (xname, cname) in GOLDENS:
        # the README's equivalence, run: the kept records under the default options give the tables the reference wrote for
        # the reduced input
        gf, gr = tl.parse_counts_text((GOLD / f"{GOLDENS[(xname, cname)]}.pss.counts.txt").read_text())
        again, _, _ = run(pkg, c, OPTS["none"], sink=False, raw=kept)
        assert np.array_equal(again.fwd, gf) and np.array_equal(again.rev, gr) and gf[2:].sum() > 0


# ---- shapes: synthetic records whose fate is known from how they are built (-q 30 against MAPQ 40 / 10) -----------------------

CONTIG = ml.clean_contig(4000, seed=5)
LONG_CONTIG = ml.clean_contig(110000, seed=6)
SYN = Case([("c", CONTIG), ("long", LONG_CONTIG)], [("c", len(CONTIG)), ("long", len(LONG_CONTIG))], [], None, [])
Q30 = OPTS["q30"]


def syn_rec(j: int, keep: bool, name_len: int = None, aux: int = 0) -> tl.Rec:
    L = 20 + j % 37
    s = 10 + (j * 7) % (len(CONTIG) - 100)
    nm = ("r%d" % j).ljust(name_len or 1 + j % 17, "x")
    r = ml.read_on(CONTIG, s, L, name=nm, rname="c", mapq=40 if keep else 10)
    return replace(r, tags=[("XZ", "Z", "a" * (aux - 1))] if aux else [])


def pattern(name: str, n: int) -> list:
    return {"none": [False] * n, "all": [True] * n, "alternating": [j % 2 == 0 for j in range(n)],
            "first": [j == 0 for j in range(n)], "last": [j == n - 1 for j in range(n)],
            "random": [bool(v) for v in np.random.default_rng(n).integers(0, 2, size=n)]}[name]


def check_synthetic(pkg, recs: list, keep: list, chunks=1, kernel=0):
    raw = tl.raw_records(SYN.refs, recs) if recs else np.zeros(0, dtype=np.uint8)
    blobs = split_records(raw)
    tabs, kept, n = run(pkg, SYN, Q30, raw=raw, chunks=chunks, kernel=kernel)
    want = b"".join(b for b, k in zip(blobs, keep) if k)
    assert kept.tobytes() == want and n == sum(keep) == tabs.stats["pss_ok"]
    return raw, blobs


COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1]
PATTERNS = ["none", "all", "alternating", "first", "last", "random"]


@pytest.mark.parametrize("n,pat", [(n, p) for n in COUNTS for p in PATTERNS if n or p == "none"])   # (an empty block has one pattern)
def test_counts_and_keep_patterns(pkg, n, pat):
    keep = pattern(pat, n)
    check_synthetic(pkg, [syn_rec(j, k) for j, k in enumerate(keep)], keep)


def test_expected_fate_of_the_synthetic_records_is_the_oracles(oracle, tmp_path):
    """the construction above (MAPQ 40 kept, MAPQ 10 dropped under -q 30) restated by the oracle"""
    keep = pattern("random", 257)
    recs = [syn_rec(j, k) for j, k in enumerate(keep)]
    fa, sam = tmp_path / "g.fa", tmp_path / "a.sam"
    tl.write_fasta(fa, SYN.contigs)
    g = oracle.load_genome(fa)
    try:
        tl.write_sam(sam, SYN.refs, recs)
        assert int(oracle.pss(g, sam, Q30.o)[2][tl.ST_OK]) == sum(keep)
        tl.write_sam(sam, SYN.refs, [r for r, k in zip(recs, keep) if not k])
        assert int(oracle.pss(g, sam, Q30.o)[2][tl.ST_OK]) == 0
    finally:
        oracle.free_genome(g)


def test_every_source_and_destination_alignment(pkg):
    """read-name and aux lengths vary so that the kept records start at every residue mod 16 in the input and in the output
    (the gather builds aligned 16-byte stores from loads at the record's own alignment)"""
    rng = np.random.default_rng(16)
    keep = [bool(v) for v in rng.integers(0, 2, size=700)]
    recs = [syn_rec(j, k, name_len=int(rng.integers(1, 18)), aux=int(rng.integers(0, 9))) for j, k in enumerate(keep)]
    _, blobs = check_synthetic(pkg, recs, keep)
    src = np.cumsum([0] + [len(b) for b in blobs])[:-1]
    dst = np.cumsum([0] + [len(b) for b, k in zip(blobs, keep) if k])[:-1]
    pairs = {(int(s) % 16, int(d) % 16) for s, d in zip(src[np.array(keep)], dst)}
    assert {p[0] for p in pairs} == set(range(16)) == {p[1] for p in pairs} and len(pairs) > 128


@pytest.mark.parametrize("long_kept", [True, False])
def test_a_record_above_64_KiB_between_short_ones(pkg, long_kept):
    big = ml.read_on(LONG_CONTIG, 50, 100000, name="long_read", rname="long", mapq=40 if long_kept else 10)
    keep = pattern("alternating", 40)
    recs = [syn_rec(j, k) for j, k in enumerate(keep)]
    recs.insert(21, big)
    keep.insert(21, long_kept)
    raw, blobs = check_synthetic(pkg, recs, keep)
    assert len(blobs[21]) > 150000


def test_second_level_of_the_scan_takes_more_than_one_round(pkg):
    """more than SUMS_ROUND tiles of SCAN_TILE records: records of one size, MAPQ set per record in the block's bytes"""
    n = SUMS_ROUND * SCAN_TILE + SCAN_TILE + 1
    one = np.frombuffer(tl.bam_record(syn_rec(3, True, name_len=6), {"c": 0, "long": 1}), dtype=np.uint8)
    keep = np.random.default_rng(3).integers(0, 4, size=n) == 0
    block = np.tile(one, n).reshape(n, one.size)
    block[:, 13] = np.where(keep, 40, 10)          # MAPQ: byte 9 of the record body
    tabs, kept, n_kept = run(pkg, SYN, Q30, raw=block.reshape(-1))
    assert n_kept == int(keep.sum()) == tabs.stats["pss_ok"] and np.array_equal(kept.reshape(-1, one.size), block[keep])


def test_three_submits_keep_the_order(pkg):
    keep = pattern("random", 3 * 257)
    check_synthetic(pkg, [syn_rec(j, k) for j, k in enumerate(keep)], keep, chunks=3)


def test_simple_kernel_path(pkg):
    keep = pattern("random", 300)
    check_synthetic(pkg, [syn_rec(j, k) for j, k in enumerate(keep)], keep, kernel=pkg.KERNEL_SIMPLE)


# ---- the submit paths ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["submit", "submit_device", "bgzf_after_genome", "bgzf_ahead_of_genome"])
def test_submit_paths(pkg, oracle, tmp_path, path):
    c, x = case_of("fuzz4401"), OPTS["q30"]
    blobs = split_records(c.raw)
    eng = pkg.Engine(pss=pss_dict(x.o))
    eng.set_record_sink()
    genome = lambda: (eng.set_genome_arrays(tl.loaded_contigs(c.contigs)), eng.set_references([n for n, _ in c.refs]))
    bam = tmp_path / "x.bam"
    try:
        if path == "submit":
            genome()
            eng.submit(c.raw)
        elif path == "submit_device":
            genome()
            hip = C.CDLL("libamdhip64.so")          # device buffers straight from the HIP runtime
            hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            offs = pkg.index_records(c.raw)
            d_r, d_o = C.c_void_p(), C.c_void_p()
            assert hip.hipMalloc(C.byref(d_r), c.raw.size + 64) == 0 and hip.hipMalloc(C.byref(d_o), offs.size * 4) == 0
            assert hip.hipMemcpy(d_r, c.raw.ctypes.data, c.raw.size, 1) == 0 and hip.hipMemcpy(d_o, offs.ctypes.data, offs.size * 4, 1) == 0
            eng.submit_device(d_r.value, c.raw.size, d_o.value, offs.size - 1)
        else:
            hb = tl.write_bam_aligned(bam, c.refs, c.recs, rng=np.random.default_rng(3))
            if path == "bgzf_after_genome":
                genome()
            else:
                eng.feed_open(len(c.refs))
            eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
            if path == "bgzf_ahead_of_genome":
                genome()
        kept = eng.finish_records()
        tabs = eng.finish()
        if path.startswith("bgzf"):
            assert eng.feed_status()["flags"] == 0
    finally:
        eng.close()
    idx = kept_indices(blobs, kept)
    fa, sam = tmp_path / "g.fa", tmp_path / "k.sam"
    tl.write_fasta(fa, c.contigs)
    g = oracle.load_genome(fa)
    try:
        tl.write_sam(sam, c.refs, c.recs)
        wf, wr, wst = oracle.pss(g, sam, x.o)
        tl.write_sam(sam, c.refs, [c.recs[i] for i in idx])
        kf, kr, _ = oracle.pss(g, sam, x.o)
    finally:
        oracle.free_genome(g)
    assert len(idx) == int(wst[tl.ST_OK]) == tabs.stats["pss_ok"] and 0 < len(idx) < len(blobs)
    assert np.array_equal(kf, wf) and np.array_equal(kr, wr) and np.array_equal(tabs.fwd, wf) and np.array_equal(tabs.rev, wr)


# ---- the contract's edges ------------------------------------------------------------------------------------------------------

def test_a_sink_that_fails_fails_the_call_and_is_not_called_again(pkg):
    keep = pattern("all", 100)
    raw = tl.raw_records(SYN.refs, [syn_rec(j, k) for j, k in enumerate(keep)])
    calls = []
    eng = pkg.Engine(pss=pss_dict(Q30.o))
    eng.set_record_sink(lambda chunk, n: calls.append(n) or 1)
    eng.set_genome_arrays(tl.loaded_contigs(SYN.contigs))
    eng.set_references([n for n, _ in SYN.refs])
    try:
        eng.submit(raw)
        with pytest.raises(pkg.PssbamError, match="record sink"):
            eng.sync()
        assert calls == [100]
        eng.submit(raw)
        tabs = eng.finish()
        assert calls == [100] and tabs.stats["pss_ok"] == 200
    finally:
        eng.close()


def _failing_engine(pkg, fail_at: int):
    """an engine over SYN whose sink returns 1 at its fail_at-th call (and records every call)"""
    calls = []
    eng = pkg.Engine(pss=pss_dict(Q30.o))
    eng.set_record_sink(lambda chunk, n: calls.append(n) or (1 if len(calls) == fail_at else 0))
    return eng, calls


def _device_idle():
    hip = C.CDLL("libamdhip64.so")
    assert hip.hipDeviceSynchronize() == 0


def test_a_sink_that_fails_at_the_second_of_three_submits(pkg):
    """A submit that reports the sink's failure does so at its top, before anything of it is queued: the caller submits the
    block again, and in the end every block has been tallied exactly once -- whichever call the failure surfaced in.  The
    device is drained in front of submit 3, so that chunk 2 is delivered (and fails) at the top of that submit."""
    blocks = [tl.raw_records(SYN.refs, [syn_rec(100 * b + j, True) for j in range(100 + b)]) for b in range(3)]
    eng, calls = _failing_engine(pkg, 2)
    eng.set_genome_arrays(tl.loaded_contigs(SYN.contigs))
    eng.set_references([n for n, _ in SYN.refs])
    failures = []
    try:
        for b, raw in enumerate(blocks):
            try:
                if b == 2:
                    _device_idle()
                    eng.submit(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint32))   # (an empty submit polls: chunk 2's copy starts)
                    _device_idle()
                eng.submit(raw)
            except pkg.PssbamError as err:
                assert "record sink" in str(err)
                failures.append(b)
                eng.submit(raw)               # nothing of the failed call was queued: the block goes in again
        try:
            tabs = eng.finish()
        except pkg.PssbamError as err:
            assert "record sink" in str(err)
            failures.append("finish")
            tabs = eng.finish()
        again = eng.finish()
    finally:
        eng.close()
    assert failures == [2] and calls == [100, 101]
    assert tabs.stats["records"] == tabs.stats["pss_ok"] == 303 and again.stats == tabs.stats


def test_a_sink_that_fails_while_submits_are_in_flight(pkg):
    """no drain: wherever the failure surfaces -- the top of a later submit, sync or finish -- it surfaces once, the sink is
    not called again, and every block is tallied exactly once (a failed submit is repeated)"""
    blocks = [tl.raw_records(SYN.refs, [syn_rec(50 * b + j, True) for j in range(60)]) for b in range(12)]
    eng, calls = _failing_engine(pkg, 3)
    eng.set_genome_arrays(tl.loaded_contigs(SYN.contigs))
    eng.set_references([n for n, _ in SYN.refs])
    failures = 0
    try:
        for raw in blocks:
            try:
                eng.submit(raw)
            except pkg.PssbamError:
                failures += 1
                eng.submit(raw)
        try:
            tabs = eng.finish()
        except pkg.PssbamError:
            failures += 1
            tabs = eng.finish()
    finally:
        eng.close()
    assert failures == 1 and calls == [60, 60, 60]
    assert tabs.stats["records"] == tabs.stats["pss_ok"] == 12 * 60


def test_a_sink_that_fails_on_the_deferred_feed(pkg, oracle, tmp_path):
    """compressed blocks fed ahead of the genome, several super-batches; the sink fails at its first chunk, inside the launches
    that set_references releases: set_references succeeds, every put-off tally runs, the failure surfaces once in finish, and
    the tables are the oracle's for the whole file"""
    c, x = case_of("fuzz4401"), OPTS["q30"]
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, c.refs, c.recs, rng=np.random.default_rng(3))
    eng, calls = _failing_engine(pkg, 1)
    failures = 0
    try:
        eng.feed_open(len(c.refs))
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
        eng.set_references([n for n, _ in c.refs])
        try:
            tabs = eng.finish()
        except pkg.PssbamError as err:
            assert "record sink" in str(err)
            failures += 1
            tabs = eng.finish()
        assert eng.feed_status()["flags"] == 0
    finally:
        eng.close()
    fa, sam = tmp_path / "g.fa", tmp_path / "a.sam"
    tl.write_fasta(fa, c.contigs)
    tl.write_sam(sam, c.refs, c.recs)
    g = oracle.load_genome(fa)
    try:
        wf, wr, wst = oracle.pss(g, sam, x.o)
    finally:
        oracle.free_genome(g)
    assert failures == 1 and len(calls) == 1
    assert np.array_equal(tabs.fwd, wf) and np.array_equal(tabs.rev, wr) and tabs.stats["records"] == len(c.recs) and tabs.stats["pss_ok"] == int(wst[tl.ST_OK])


def test_sink_must_be_set_before_the_first_submit(pkg):
    raw = tl.raw_records(SYN.refs, [syn_rec(0, True)])
    eng = pkg.Engine(pss=pss_dict(Q30.o))
    eng.set_genome_arrays(tl.loaded_contigs(SYN.contigs))
    eng.set_references([n for n, _ in SYN.refs])
    try:
        eng.submit(raw)
        with pytest.raises(pkg.PssbamError):
            eng.set_record_sink()
        eng.reset()
        eng.set_record_sink()
        eng.submit(raw)
        assert eng.finish_records().tobytes() == raw.tobytes()
    finally:
        eng.close()
    fk = pkg.Engine(kmer=dict(klen=4))
    try:
        with pytest.raises(pkg.PssbamError):
            fk.set_record_sink()
    finally:
        fk.close()


def test_without_a_sink_the_launch_count_is_the_one_before_the_feature(pkg):
    contigs, refs, recs = tl.fuzz_dataset(*LAUNCH_INPUT)
    eng = pkg.Engine(pss=dict(region_len=15))
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([n for n, _ in refs])
    try:
        eng.kernel_time()
        eng.submit(tl.raw_records(refs, recs))
        eng.sync()
        assert eng.kernel_time()[1] == LAUNCHES_BEFORE_THE_SINK
    finally:
        eng.close()

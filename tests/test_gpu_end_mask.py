"""The end mask (pssbam_engine_set_end_mask, pss-bam -K) on the GPU, through the Engine wrapper: what a sink receives with the
mask on is end_mask_lib.mask_record -- the definition restated on BAM bytes -- applied to what the same engine delivers with
the mask off, record for record; and nothing else of the run moves: tables, status counters, the tally's launch count.

The restatement takes the unmasked stream as its input, so the selection is not tested again here (tests/test_gpu_select.py);
that the crafted set's special records are among the kept ones is checked against the CPU oracle."""
from dataclasses import dataclass, replace
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import deflate_lib as dl
import end_mask_lib as em
import gapped_lib as gl
import mismatch_lib as ml
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
SCAN_TILE = 1024          # csrc/select_kernels.h SELECT_SCAN_TILE
COMBOS = [(m, n5, n3) for m in em.MODES for n5, n3 in em.WIDTHS]
EINVAL, ESTATE = "pssbam error -1:", "pssbam error -5:"


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    assert hasattr(p.hip_lib(), "pssbam_engine_set_end_mask")
    return p


@dataclass
class Case:
    contigs: list
    refs: list
    raw: np.ndarray
    pss: dict
    gapped: bool = False


def golden_case(base: str) -> Case:
    fa_txt = (GOLD / f"{base}.fa").read_text()
    contigs = [(blk.split("\n", 1)[0].split()[0], "".join(blk.split("\n")[1:])) for blk in fa_txt.split(">")[1:]]
    refs, raw = tl.read_bam(GOLD / f"{base}.bam")
    return Case(contigs, refs, raw, dict(region_len=15))


_CASES: dict = {}


def case_of(name: str) -> Case:
    if name not in _CASES:
        if name == "crafted":
            _CASES[name] = Case(em.CONTIGS, em.REFS, em.crafted()[1], dict(region_len=em.REGION_LEN, min_mq=em.MIN_MQ), gapped=True)
        elif name.startswith("set"):
            _CASES[name] = golden_case(name)
        else:
            contigs, refs, recs = tl.fuzz_dataset(int(name[4:]), 1500)
            _CASES[name] = Case(contigs, refs, tl.raw_records(refs, recs), dict(region_len=15, min_mq=30))
    return _CASES[name]


def run(pkg, c: Case, mask=None, sink="record", raw=None, chunks=1):
    """-> (Tables, the sink's bytes or None, launch count of kernel_time, records / block totals the sink reported)"""
    raw = c.raw if raw is None else raw
    eng = pkg.Engine(pss=c.pss)
    try:
        if c.gapped:
            eng.set_gapped(True)
        if sink == "record":
            eng.set_record_sink()
        elif sink == "block":
            eng.set_block_sink()
        if mask is not None:
            eng.set_end_mask(*mask)
        eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
        eng.set_references([n for n, _ in c.refs])
        eng.kernel_time()
        offs = pkg.index_records(raw)
        n = offs.size - 1
        cuts = [n * i // chunks for i in range(chunks + 1)]
        for a, b in zip(cuts[:-1], cuts[1:]):
            if b > a:
                o = offs[a:b + 1].astype(np.int64)
                eng.submit(raw[o[0]:o[-1]], (o - o[0]).astype(np.uint32))
        got = eng.finish_records() if sink == "record" else eng.finish_blocks() if sink == "block" else None
        said = eng.records_kept if sink == "record" else eng.blocks_kept if sink == "block" else None
        launches = eng.kernel_time()[1]
        return eng.finish(), got, launches, said
    finally:
        eng.close()


_PLAIN: dict = {}


def plain(pkg, name: str):
    """the run of the case with a record sink and no mask, once"""
    if name not in _PLAIN:
        _PLAIN[name] = run(pkg, case_of(name))
    return _PLAIN[name]


def same_run(a, b):
    return np.array_equal(a[0].fwd, b[0].fwd) and np.array_equal(a[0].rev, b[0].rev) and a[0].stats == b[0].stats and a[2] == b[2]


# ---- 4: every mode on the record sink ---------------------------------------------------------------------------------------------

def test_the_crafted_sets_special_records_are_kept(pkg, oracle, tmp_path):
    """what the masked runs below are about is in the stream: short reads of every length, both strands, the clipped reads,
    the read without qualities; the count is the CPU oracle's under -q 20 -r 1 on the anchored records (-I)"""
    recs, raw, bad = em.crafted()
    _, kept, _, n_kept = plain(pkg, "crafted")
    blobs = em.split_records(kept)
    fa, sam = tmp_path / "g.fa", tmp_path / "a.sam"
    tl.write_fasta(fa, em.CONTIGS)
    tl.write_sam(sam, em.REFS, gl.anchor_recs(recs))
    g = oracle.load_genome(fa)
    try:
        st = oracle.pss(g, sam, tl.PssOpts(region_len=em.REGION_LEN, min_mq=em.MIN_MQ))[2]
    finally:
        oracle.free_genome(g)
    assert len(blobs) == n_kept == int(st[tl.ST_OK]) and 100 < n_kept < len(recs)
    names = {b[36:36 + b[12] - 1].decode() for b in blobs}
    assert {"softclip", "hardclip", "noqual1"} <= names and "malformed" not in names
    lay = [em.layout(b) for b in blobs]
    assert {(l, rev) for l, rev, *_ in lay} >= {(l, rev) for l in em.LENGTHS for rev in (False, True)}
    assert sum(1 for b, (l, _, _, q, _) in zip(blobs, lay) if l and b[q] == 0xFF) == 1
    all_blobs = em.split_records(raw)
    assert len(kept) < len(raw) and all(b in all_blobs for b in blobs)


@pytest.mark.parametrize("mode,n5,n3", COMBOS)
@pytest.mark.parametrize("name", ["crafted", "setA", "setD", "fuzz4401"])
def test_record_sink_delivers_the_masked_records(pkg, name, mode, n5, n3):
    base = plain(pkg, name)
    got = run(pkg, case_of(name), mask=(mode, n5, n3))
    want = em.mask_stream(base[1], mode, n5, n3)
    assert got[1].tobytes() == want and got[3] == base[3] > 0
    assert same_run(got, base)
    assert want != base[1].tobytes()


def test_the_tables_are_those_of_the_run_without_a_sink(pkg):
    c = case_of("setD")
    bare = run(pkg, c, sink=None)
    assert same_run(bare, plain(pkg, "setD")) and same_run(bare, run(pkg, c, mask=("all", 5, 5)))


# ---- 5: the block sink -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,mode,n5,n3", [("crafted", *c) for c in COMBOS] + [(n, "ds", 5, 5) for n in ("setA", "setD", "fuzz4401")])
def test_block_sink_deflates_the_masked_stream(pkg, name, mode, n5, n3):
    base = plain(pkg, name)
    tabs, data, launches, said = run(pkg, case_of(name), mask=(mode, n5, n3), sink="block")
    want = em.mask_stream(base[1], mode, n5, n3)
    blocks = dl.check_fixed_cut(data.tobytes(), want)          # magic, BSIZE chain, CRC-32, ISIZE, the cut every 0xFF00 bytes
    assert said == dict(n_blocks=len(blocks), raw_bytes=len(want), n_records=base[3])
    assert same_run((tabs, None, launches), base)


# ---- 6: the cut --------------------------------------------------------------------------------------------------------------------

def syn_raw(n: int, every_second_dropped: bool):
    """n reads of 20..56 bases over the crafted contig, names of 1..17 bytes, MAPQ 40 -- or 10, below the crafted case's -q, on
    every second one; -> (raw, the blobs that are kept)"""
    recs = []
    for j in range(n):
        L = 20 + j % 37
        r = ml.read_on(em.CONTIG, 10 + (j * 7) % (len(em.CONTIG) - 100), L, name=("s%dxxxxxxxxxxxxxxxxx" % j)[:1 + j % 17], flag=16 * (j % 3 == 0),
                       rname="c", tlen=L, mapq=10 if every_second_dropped and j % 2 else 40)
        recs.append(replace(r, tags=[("XZ", "Z", "a" * (j % 5))] if j % 4 == 3 else []))
    blobs = [tl.bam_record(r, {"c": 0}) for r in recs]
    return np.frombuffer(b"".join(blobs), dtype=np.uint8), [b for j, b in enumerate(blobs) if not (every_second_dropped and j % 2)]


@pytest.mark.parametrize("dropped", [False, True])
@pytest.mark.parametrize("n", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_the_cut_into_submits_does_not_show(pkg, n, dropped):
    """1, 3 and 7 submits (with 3 and 7 both output buffers are in flight): the same masked stream, which is the restatement on
    the records known to be kept by how they were built"""
    raw, kept = syn_raw(n, dropped)
    want = b"".join(em.mask_record(b, "ds", 5, 5) for b in kept)
    assert want != b"".join(kept)
    for chunks in (1, 3, 7):
        tabs, got, _, n_kept = run(pkg, case_of("crafted"), mask=("ds", 5, 5), raw=raw, chunks=chunks)
        assert got.tobytes() == want and n_kept == len(kept) == tabs.stats["pss_ok"], chunks


# ---- 7: the file is what pss-bam sees it as ------------------------------------------------------------------------------------------

def test_masked_ends_are_missing_from_the_tables_of_the_masked_file(pkg, oracle, tmp_path):
    """setD masked with all,2,3 and tallied by the CPU oracle.  oracle/pss_oracle.c: row i + 2 of the forward table pairs read
    position i from the 5' end -- stored index i on a forward, L - 1 - i on a reverse read -- with the reference, row i + 2 of
    the reverse table position i from the 3' end -- stored L - 1 - i on a forward, i on a reverse read; a read base N adds
    nothing.  Those are the mask's regions, so rows 2, 3 of the forward and rows 2, 3, 4 of the reverse table are zero.  L is
    |TLEN|; where it is not the length of SEQ (mates), the position lies beyond SEQ and adds nothing either way, or is the
    stored index i that the mask covers (tally_fwd on a forward first mate, tally_rev on a reverse second mate).  Every other
    row is the unmasked file's as long as the reads are at least region_len + 3 long -- a position row then never reaches the
    other end's region; setD's shortest read has 15 bases, hence -r 10 (with -r 15 its 15..17-base reads would thin rows up
    to 16)."""
    c = case_of("setD")
    _, recs = ml.read_sam(GOLD / "setD.sam")
    o = tl.PssOpts(region_len=10)
    assert min(len(r.seq) for r in recs) >= o.region_len + 3
    cc = replace(c, pss=dict(region_len=10))
    base = run(pkg, cc)
    got = run(pkg, cc, mask=("all", 2, 3))
    kept, j, all_blobs = [], 0, em.split_records(c.raw)
    for b in em.split_records(base[1]):                   # the kept records are a subsequence of the input
        while all_blobs[j] != b:
            j += 1
        kept.append(recs[j])
        j += 1
    masked = [replace(r, seq=em.seq_qual(b)[0], qual=em.seq_qual(b)[1]) for r, b in zip(kept, em.split_records(got[1]))]
    assert len(masked) == len(kept) > 300 and all(m.seq[3:-3] == k.seq[3:-3].upper() and len(m.seq) == len(k.seq) for m, k in zip(masked, kept))
    g = oracle.load_genome(GOLD / "setD.fa")
    try:
        sam = tmp_path / "k.sam"
        tl.write_sam(sam, c.refs, kept)
        f0, r0, s0 = oracle.pss(g, sam, o)
        tl.write_sam(sam, c.refs, masked)
        f1, r1, s1 = oracle.pss(g, sam, o)
    finally:
        oracle.free_genome(g)
    assert int(s0[tl.ST_OK]) == int(s1[tl.ST_OK]) == len(kept)
    assert f0[2:4].sum() > 0 and r0[2:5].sum() > 0 and not f1[2:4].any() and not r1[2:5].any()
    assert np.array_equal(np.delete(f1, [2, 3], 0), np.delete(f0, [2, 3], 0)) and np.array_equal(np.delete(r1, [2, 3, 4], 0), np.delete(r0, [2, 3, 4], 0))
    assert np.array_equal(base[0].fwd, f0) and np.array_equal(base[0].rev, r0)       # (and the engine's own tables are the unmasked file's)
    assert np.array_equal(got[0].fwd, f0) and np.array_equal(got[0].rev, r0)


# ---- 8: the setter's contract --------------------------------------------------------------------------------------------------------

def test_setter_contract(pkg):
    c = case_of("setD")
    base = plain(pkg, "setD")
    eng = pkg.Engine(pss=c.pss)
    try:
        for bad in [(4, 1, 1), (-1, 1, 1), (1, 0, 0), (2, 0, 0), (3, 0, 0), (1, 65536, 1), (1, 1, 65536), (0, 70000, 0), (1, -1, 2)]:
            with pytest.raises(pkg.PssbamError, match=EINVAL):
                eng.set_end_mask(*bad)
        eng.set_end_mask("all", 65535, 65535)
        eng.set_end_mask("ds", 0, 1)
        eng.set_end_mask(None, 0, 0)
        eng.set_end_mask("ss", 2)                          # before the sink: legal
        eng.set_record_sink()
        eng.set_end_mask("all", 2, 3)                      # and after it
        eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
        eng.set_references([n for n, _ in c.refs])
        eng.submit(c.raw)
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.set_end_mask("all", 1, 1)
        with pytest.raises(pkg.PssbamError, match=ESTATE):
            eng.set_end_mask(None, 0, 0)
        want = em.mask_stream(base[1], "all", 2, 3)
        assert eng.finish_records().tobytes() == want
        eng.reset()                                        # the setting survives
        eng.submit(c.raw)
        assert eng.finish_records().tobytes() == want
        eng.reset()
        eng.set_end_mask("ds", 5)                          # legal again after reset; n3 defaults to n5
        eng.submit(c.raw)
        assert eng.finish_records().tobytes() == em.mask_stream(base[1], "ds", 5, 5)
    finally:
        eng.close()


@pytest.mark.parametrize("sink", ["record", "block", None])
def test_mode_off_is_the_run_without_the_call(pkg, sink):
    c = case_of("setD")
    a, b = run(pkg, c, sink=sink), run(pkg, c, sink=sink, mask=(None, 0, 0))
    assert same_run(a, b) and a[3] == b[3]
    if sink:
        assert a[1].tobytes() == b[1].tobytes() and a[1].size > 0
    if sink is None:                                       # a mask without a sink: nothing to act on, nothing launched for it
        assert same_run(a, run(pkg, c, sink=None, mask=("all", 5, 5)))

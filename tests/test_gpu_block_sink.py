"""The block sink (pssbam_engine_set_block_sink, pss-bam -O ... -Z) on the GPU: what it delivers is a whole number of complete
BGZF blocks -- judged by deflate_lib.walk, Python's zlib -- that inflate to exactly the byte stream the RECORD sink delivers for
the same input and settings, cut every 0xFF00 bytes within each chunk.  tests/test_gpu_select.py ties the record sink to the
oracle; its record sets, option sets and synthetic records are imported from there.  Where the fate of the records is known
from how they are built (MAPQ 40 kept, MAPQ 10 dropped under -q 30) the expected bytes are put together here."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest

import deflate_lib as dl
import mismatch_lib as ml
import pssbam_testlib as tl
import test_gpu_select as sel
from test_gpu_select import pkg  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

P = dl.PAYLOAD
OPTS = {
    "plain": sel.OPTS["none"],
    "q20_T": sel.Opt(tl.PssOpts(min_mq=20), setup=sel._set_regions),
    "y3_Q20": sel.OPTS["y3_Q20"],
}
CASES = ["setA", "fuzz4401"]
PATHS = ["submit", "submit_device", "submit_bgzf"]


class Collected:
    """what a sink was handed: the chunks and the sums of the counts"""
    def __init__(self):
        self.chunks, self.n_blocks, self.raw_bytes, self.n_records = [], 0, 0, 0


def run(pkg, c, x, sink, path="submit", chunks=1, raw=None, tmp_path=None):
    """-> (Tables, Collected or None, kernel_time's launch count); sink: "block", "record" or None"""
    raw = c.raw if raw is None else raw
    got = Collected()
    eng = pkg.Engine(pss=sel.pss_dict(x.o), read_group=x.rg)
    if x.setup:
        x.setup(eng, c)

    def on_blocks(chunk, n_blocks, raw_bytes, n_records):
        walked = dl.walk(chunk.tobytes())      # every hand-over is whole blocks, cut every 0xFF00 bytes of the chunk
        assert len(walked) == n_blocks == -(-raw_bytes // P) and n_records > 0
        assert [len(p) for _, p in walked] == [min(P, raw_bytes - k * P) for k in range(n_blocks)]
        got.chunks.append(b"".join(p for _, p in walked))
        got.n_blocks, got.raw_bytes, got.n_records = got.n_blocks + n_blocks, got.raw_bytes + raw_bytes, got.n_records + n_records

    def on_records(chunk, n_records):
        got.chunks.append(chunk.tobytes())
        got.raw_bytes, got.n_records = got.raw_bytes + chunk.size, got.n_records + n_records

    if sink == "block":
        eng.set_block_sink(on_blocks)
    elif sink == "record":
        eng.set_record_sink(on_records)
    eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
    eng.set_references([n for n, _ in c.refs])
    freed = []
    try:
        eng.kernel_time()
        if path == "submit_bgzf":
            bam = tmp_path / "in.bam"
            hb = tl.write_bam_aligned(bam, c.refs, c.recs, rng=np.random.default_rng(3))
            eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        else:
            offs = pkg.index_records(raw)
            n = offs.size - 1
            cuts = [n * i // chunks for i in range(chunks + 1)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                if b <= a:
                    continue
                o = offs[a:b + 1].astype(np.int64)
                part, po = np.ascontiguousarray(raw[o[0]:o[-1]]), (o - o[0]).astype(np.uint32)
                if path == "submit":
                    eng.submit(part, po)
                else:
                    hip = C.CDLL("libamdhip64.so")
                    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
                    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
                    hip.hipFree.argtypes = [C.c_void_p]
                    d_r, d_o = C.c_void_p(), C.c_void_p()
                    assert hip.hipMalloc(C.byref(d_r), part.size + 64) == 0 and hip.hipMalloc(C.byref(d_o), po.size * 4) == 0
                    freed += [(hip, d_r), (hip, d_o)]
                    assert hip.hipMemcpy(d_r, part.ctypes.data, part.size, 1) == 0 and hip.hipMemcpy(d_o, po.ctypes.data, po.size * 4, 1) == 0
                    eng.submit_device(d_r.value, part.size, d_o.value, po.size - 1)
        eng.sync()
        launches = eng.kernel_time()[1]
        tabs = eng.finish()
        if path == "submit_bgzf":
            assert eng.feed_status()["flags"] == 0
        return tabs, (got if sink else None), launches
    finally:
        eng.close()
        for hip, p in freed:
            hip.hipFree(p)


_RECORD_RUNS: dict = {}


def record_run(pkg, cname, xname, path, tmp_path):
    """the record sink's stream for this input, once per module"""
    key = (cname, xname, path)
    if key not in _RECORD_RUNS:
        _RECORD_RUNS[key] = run(pkg, sel.case_of(cname), OPTS[xname], "record", path, tmp_path=tmp_path)
    return _RECORD_RUNS[key]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("xname", list(OPTS))
@pytest.mark.parametrize("cname", CASES)
def test_blocks_inflate_to_the_record_sinks_stream(pkg, tmp_path, cname, xname, path):
    c, x = sel.case_of(cname), OPTS[xname]
    rt, rgot, _ = record_run(pkg, cname, xname, path, tmp_path)
    bt, bgot, b_launches = run(pkg, c, x, "block", path, tmp_path=tmp_path)
    want = b"".join(rgot.chunks)
    assert 0 < len(want) < c.raw.size or xname == "plain"
    assert b"".join(bgot.chunks) == want
    assert bgot.n_records == rgot.n_records == len(sel.split_records(np.frombuffer(want, dtype=np.uint8)))
    assert bgot.raw_bytes == len(want)
    # tables, status counters and the launch count: those of the run without a sink
    pt, _, p_launches = run(pkg, c, x, None, path, tmp_path=tmp_path)
    assert np.array_equal(bt.fwd, pt.fwd) and np.array_equal(bt.rev, pt.rev) and bt.stats == pt.stats and bt.stats == rt.stats
    assert b_launches == p_launches > 0


@pytest.mark.parametrize("chunks", [1, 2, 7])
def test_the_inflated_stream_does_not_depend_on_the_cut_into_submits(pkg, chunks):
    c, x = sel.case_of("fuzz4401"), OPTS["q20_T"]
    _, rgot, _ = record_run(pkg, "fuzz4401", "q20_T", "submit", None)
    _, bgot, _ = run(pkg, c, x, "block", chunks=chunks)
    assert b"".join(bgot.chunks) == b"".join(rgot.chunks) and (1 if chunks == 1 else 2) <= len(bgot.chunks) <= chunks


def synthetic(pkg, recs, keep, chunks=1):
    raw = tl.raw_records(sel.SYN.refs, recs)
    blobs = sel.split_records(raw)
    tabs, got, _ = run(pkg, sel.SYN, sel.Q30, "block", raw=raw, chunks=chunks)
    want = b"".join(b for b, k in zip(blobs, keep) if k)
    assert b"".join(got.chunks) == want and got.n_records == sum(keep) == tabs.stats["pss_ok"] and got.raw_bytes == len(want)
    return got, blobs


def test_nothing_kept_delivers_nothing(pkg):
    keep = [False] * 300
    got, _ = synthetic(pkg, [sel.syn_rec(j, k) for j, k in enumerate(keep)], keep)
    assert got.chunks == [] and got.n_blocks == 0


def test_one_record_spans_three_blocks(pkg):
    big = ml.read_on(sel.LONG_CONTIG, 50, 100000, name="long_read", rname="long", mapq=40)
    keep = sel.pattern("alternating", 40)
    recs = [sel.syn_rec(j, k) for j, k in enumerate(keep)]
    recs.insert(21, big)
    keep.insert(21, True)
    got, blobs = synthetic(pkg, recs, keep)
    assert len(blobs[21]) > 150000 and got.n_blocks == 3
    first = sum(len(b) for b, k in zip(blobs[:21], keep) if k)
    assert first < P and first + len(blobs[21]) > 2 * P      # it starts in block 0 and ends in block 2


@pytest.mark.parametrize("total", [P - 1, P, P + 1])
def test_kept_totals_around_one_block(pkg, total):
    """kept and dropped records alternate; the last kept record's Z field is padded until the kept bytes are `total`"""
    recs, keep, size = [], [], 0
    idx = {n: i for i, (n, _) in enumerate(sel.SYN.refs)}
    j = 0
    while True:
        r = sel.syn_rec(j, True)
        n = len(tl.bam_record(r, idx))
        if size + n + 144 > total:            # (what is left takes the last record, some 135 bytes at most, and an empty Z field)
            break
        recs += [r, sel.syn_rec(j + 1, False)]
        keep += [True, False]
        size += n
        j += 2
    last = sel.syn_rec(j, True, name_len=5)
    bare = len(tl.bam_record(last, idx))
    pad = total - size - bare                  # the tag takes 3 bytes, its text pad - 4 and the NUL
    assert pad >= 4
    last = replace(last, tags=[("XZ", "Z", "a" * (pad - 4))])
    assert size + len(tl.bam_record(last, idx)) == total
    got, _ = synthetic(pkg, recs + [last], keep + [True])
    assert got.raw_bytes == total and got.n_blocks == (2 if total > P else 1)


def test_a_sink_that_fails_fails_the_call_and_is_not_called_again(pkg):
    raw = tl.raw_records(sel.SYN.refs, [sel.syn_rec(j, True) for j in range(100)])
    calls = []
    eng = pkg.Engine(pss=sel.pss_dict(sel.Q30.o))
    eng.set_block_sink(lambda chunk, n_blocks, raw_bytes, n: calls.append(n) or 1)
    eng.set_genome_arrays(tl.loaded_contigs(sel.SYN.contigs))
    eng.set_references([n for n, _ in sel.SYN.refs])
    try:
        eng.submit(raw)
        with pytest.raises(pkg.PssbamError, match="block sink"):
            eng.sync()
        assert calls == [100]
        eng.submit(raw)
        tabs = eng.finish()
        assert calls == [100] and tabs.stats["pss_ok"] == 200
    finally:
        eng.close()


def test_one_sink_or_the_other(pkg):
    for first, second in (("set_record_sink", "set_block_sink"), ("set_block_sink", "set_record_sink")):
        eng = pkg.Engine(pss=sel.pss_dict(sel.Q30.o))
        try:
            getattr(eng, first)()
            with pytest.raises(pkg.PssbamError, match="pssbam error -1"):
                getattr(eng, second)()
            getattr(eng, first)(None)           # switched off: the other one may be set
            getattr(eng, second)()
        finally:
            eng.close()
    fk = pkg.Engine(kmer=dict(klen=4))
    try:
        with pytest.raises(pkg.PssbamError):
            fk.set_block_sink()
    finally:
        fk.close()


def test_set_before_the_first_submit_and_kept_across_reset(pkg):
    raw = tl.raw_records(sel.SYN.refs, [sel.syn_rec(j, True) for j in range(50)])
    eng = pkg.Engine(pss=sel.pss_dict(sel.Q30.o))
    eng.set_genome_arrays(tl.loaded_contigs(sel.SYN.contigs))
    eng.set_references([n for n, _ in sel.SYN.refs])
    try:
        eng.submit(raw)
        with pytest.raises(pkg.PssbamError):
            eng.set_block_sink()
        eng.reset()
        eng.set_block_sink()
        eng.submit(raw)
        one = eng.finish_blocks().tobytes()
        assert b"".join(p for _, p in dl.walk(one)) == raw.tobytes() and eng.blocks_kept == {"n_blocks": 1, "raw_bytes": raw.size, "n_records": 50}
        eng.reset()
        eng.submit(raw)
        assert eng.finish_blocks().tobytes() == one     # the same input in the same submits: the same bytes
    finally:
        eng.close()

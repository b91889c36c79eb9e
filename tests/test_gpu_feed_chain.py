"""The device record index (the bgzf_chain_* kernels of csrc/inflate_kernels.h, the super- and sub-batch cutting of
csrc/bgzf_api.h) on the crafted block layouts and streams of feed_chain_lib.py, through the default inflate path.

One checker for every case: the records the index found -- delivered by the record sink behind submit_bgzf, byte for byte
and in input order -- must be the serial walk's, the status flags the stated ones, the record count the walk's, and the
tables those of a host-path run (Engine.submit) of the same records.  Every comparison is exact.  Where the input is built
to reach bgzf_chain_repair, PSSBAM_FEED_REPAIR=0 must raise PSSBAM_FEED_RAGGED on it.  test_feed_chain_host.py shows on the
CPU that each stream is what its case claims."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import feed_chain_lib as fc
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu
PSS, KMER = dict(region_len=12), dict(klen=4)
FEED_ENV = ("PSSBAM_FEED_SUPER_BYTES", "PSSBAM_FEED_SUB_BYTES", "PSSBAM_FEED_REPAIR")


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


def _engine(pkg, c, dup=False, cov=False, sink=True):
    eng = pkg.Engine(pss=PSS, kmer=None if dup else KMER)      # (duplicate flagging is not for an engine with both tallies)
    if dup:
        eng.set_duplicates(True)
    if cov:
        eng.set_coverage(True)
    if sink:
        eng.set_record_sink()
    eng.set_genome_arrays(tl.loaded_contigs(c.contigs))
    eng.set_references([n for n, _ in c.refs])
    return eng


def _results(eng, c, dup, cov):
    out = {"sink": eng.finish_records().tobytes()}
    t = eng.finish()
    out.update(fwd=t.fwd, rev=t.rev, k5=t.k5, k3=t.k3, records=t.stats["records"])
    if dup:
        out["dup"] = eng.finish_duplicates()
    if cov:
        out["cov"] = eng.finish_coverage(len(c.refs))
    return out


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


_HOST = {}


def _host(pkg, c, records: bytes, dup=False, cov=False):
    """the host path on the walk's records, once per stream and setting"""
    key = (c.name, len(records), dup, cov)
    if key not in _HOST:
        eng = _engine(pkg, c, dup, cov)
        try:
            eng.submit(np.frombuffer(records, dtype=np.uint8))
            _HOST[key] = _results(eng, c, dup, cov)
        finally:
            eng.close()
    return _HOST[key]


def _set_env(monkeypatch, env):
    for k in FEED_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _compare(got, want, flags, want_flags, records, plain, what):
    assert flags == want_flags, (what, flags)
    if plain:
        assert got["sink"] == records, what                   # the serial walk's records, whole, in order
    assert got["sink"] == want["sink"], what
    assert got["records"] == want["records"], what
    for k in ("fwd", "rev", "k5", "k3", "dup", "cov"):
        assert _same(got.get(k), want.get(k)), (what, k)


def check(pkg, monkeypatch, c, env=None, max_batch=None, dup=False, cov=False):
    records = b"".join(fc.records_of(c)[0])
    want = _host(pkg, c, records, dup, cov)
    assert want["records"] == c.n_records and (dup or want["sink"] == records)   # the engine keeps every record of the stream
    _set_env(monkeypatch, c.env if env is None else env)
    eng = _engine(pkg, c, dup, cov)
    try:
        eng.submit_bgzf(np.frombuffer(c.bgzf()[0], dtype=np.uint8), header_bytes=c.head_len,
                        max_batch_inflated=max_batch or c.max_batch)
        flags = eng.feed_status()["flags"]
        got = _results(eng, c, dup, cov)
    finally:
        eng.close()
    _compare(got, want, flags, c.flags, records, not dup, (c.name, env, max_batch, dup, cov))
    return got


def ragged_without_repair(pkg, monkeypatch, c):
    """the input does reach bgzf_chain_repair: switched off, it leaves PSSBAM_FEED_RAGGED standing"""
    _set_env(monkeypatch, {**c.env, "PSSBAM_FEED_REPAIR": "0"})
    eng = _engine(pkg, c, sink=False)
    try:
        eng.submit_bgzf(np.frombuffer(c.bgzf()[0], dtype=np.uint8), header_bytes=c.head_len, max_batch_inflated=c.max_batch)
        assert eng.feed_status()["flags"] & 2, c.name
    finally:
        eng.close()


@pytest.mark.parametrize("env,max_batch", [({}, 1 << 30), (fc.SUPER_1M, 3000), (fc.SUPER_1M, 700)])
def test_tiny_blocks(pkg, monkeypatch, env, max_batch):
    """case 1: length words over two to four blocks, candidates a few bytes before a block's end, empty blocks and an EOF
    block mid-stream; as one submit and as submits that cut inside records"""
    check(pkg, monkeypatch, fc.tiny_blocks(), env, max_batch)


@pytest.mark.parametrize("make", [fc.false_start_inside, fc.four_decoys, fc.broken_behind_anchor, fc.broken_far_apart,
                                  fc.broken_twice_in_a_row, fc.broken_at_super_end])
def test_repair(pkg, monkeypatch, make):
    """cases 2, 3 and 4: a fake chain taken in front of the true start in its block; a block whose four tries go to decoys;
    broken links behind the anchor, 64 and more blocks apart, in two blocks running, and at the end of a super-batch where
    the fake record is first taken for the tail"""
    c = make()
    check(pkg, monkeypatch, c)
    ragged_without_repair(pkg, monkeypatch, c)


@pytest.mark.parametrize("trailer", [False, True])
def test_fake_chain_inside_a_long_record(pkg, monkeypatch, trailer):
    """case 5: the repair walk marks whole blocks "none"; the fake chain ends on the host record's end, or does not"""
    c = fc.inside_long_record(trailer)
    check(pkg, monkeypatch, c)
    check(pkg, monkeypatch, c, fc.SUPER_1M, 2000)
    ragged_without_repair(pkg, monkeypatch, c)


@pytest.mark.parametrize("with_fakes", [False, True])
def test_record_over_several_super_batches(pkg, monkeypatch, with_fakes):
    """case 6: super-batches in which no record starts, the carry growing from one to the next; with fake chains in one"""
    c = fc.record_2_5_mib(with_fakes)
    check(pkg, monkeypatch, c)
    if with_fakes:
        ragged_without_repair(pkg, monkeypatch, c)


def test_record_of_16_mib(pkg, monkeypatch):
    """case 7: block_size == 1 << 24 is indexed on the device, exactly"""
    check(pkg, monkeypatch, fc.record_16_mib(0))


def test_record_above_16_mib_goes_the_host_way(pkg, monkeypatch, tmp_path):
    """case 7: block_size == (1 << 24) + 1 raises PSSBAM_FEED_RAGGED, and bin/pss-bam, which then reads the file on the host,
    writes the counts file of a run that never used the device feed: the fallback loses no record"""
    c = fc.record_16_mib(1)
    _set_env(monkeypatch, {})
    eng = _engine(pkg, c, sink=False)
    try:
        eng.submit_bgzf(np.frombuffer(c.bgzf()[0], dtype=np.uint8), header_bytes=c.head_len)
        assert eng.feed_status()["flags"] & 2
    finally:
        eng.close()
    fa, bam = tmp_path / "g.fa", tmp_path / "a.bam"
    tl.write_fasta(fa, c.contigs)
    bam.write_bytes(c.bgzf()[0])
    texts = []
    for k, extra in enumerate(({}, {"PSSBAM_DEVICE_INFLATE": "0"})):
        pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-F", str(fa), "-B", str(bam), "-o", str(tmp_path / "o")]
                            + tl.PssOpts(region_len=12).argv(), capture_output=True, text=True,
                            env={**os.environ, "PSSBAM_STATS": "1", **extra})
        assert pr.returncode == 0, pr.stderr[-3000:]
        assert ("falling back to the host reader" in pr.stderr) == (k == 0), pr.stderr[-3000:]
        assert f"[pssbam] records={c.n_records}" in pr.stderr, pr.stderr[-3000:]
        texts.append((tmp_path / "o.pss.counts.txt").read_text())
        (tmp_path / "o.pss.counts.txt").unlink()
    assert texts[0] == texts[1]
    fwd, rev = tl.parse_counts_text(texts[0])
    assert int(fwd.sum()) + int(rev.sum()) > 0


def _break_run(pkg, monkeypatch, cx, cy, want_flags, breaks=1, before=0):
    rx, ry = (b"".join(fc.records_of(c)[0]) for c in (cx, cy))
    want = _host(pkg, cx, rx + ry)
    _set_env(monkeypatch, {})
    eng = _engine(pkg, cx)
    try:
        for _ in range(before):
            eng.feed_break()                                   # on an engine that was never fed: nothing to break
        eng.submit_bgzf(np.frombuffer(cx.bgzf()[0], dtype=np.uint8), header_bytes=cx.head_len)   # (pending: not flushed yet)
        for _ in range(breaks):
            eng.feed_break()
        eng.submit_bgzf(np.frombuffer(cy.bgzf()[0], dtype=np.uint8), header_bytes=cy.head_len)
        flags = eng.feed_status()["flags"]
        got = _results(eng, cx, False, False)
    finally:
        eng.close()
    _compare(got, want, flags, want_flags, rx + ry, True, (cx.name, cy.name, breaks, before))


@pytest.mark.parametrize("cut_inside,headerless,breaks,before", [(True, False, 1, 0), (False, False, 1, 0), (True, True, 1, 0),
                                                                 (True, False, 2, 1), (False, True, 2, 2)])
def test_feed_break(pkg, monkeypatch, cut_inside, headerless, breaks, before):
    """case 8: stream X, a break, stream Y.  X's whole records and all of Y's, exactly; PSSBAM_FEED_TRUNCATED if and only if X
    was cut inside a record; Y is walked from its first byte (behind its header, or -- headerless -- from byte 0, where X's
    cut record would otherwise have gone on); a break twice in a row or on an engine never fed changes nothing"""
    cx, cy, cy0 = fc.break_streams(cut_inside)
    _break_run(pkg, monkeypatch, cx, cy0 if headerless else cy, 8 if cut_inside else 0, breaks, before)


def test_feed_break_on_an_engine_never_fed(pkg):
    c = fc.tiny_blocks()
    eng = _engine(pkg, c)
    try:
        eng.feed_break()
        eng.feed_break()
        assert eng.feed_status()["flags"] == 0 and eng.finish_records().size == 0
    finally:
        eng.close()


@pytest.mark.parametrize("make", [fc.sub_ragged, fc.sub_long])
@pytest.mark.parametrize("mode", ["plain", "duplicates", "coverage"])
def test_sub_batches(pkg, monkeypatch, make, mode):
    """case 9: tally sub-batches of 128 KiB (PSSBAM_FEED_SUB_BYTES): records that cross their bounds, sub-batches in which no
    record starts; the select, duplicate and coverage kernels per sub-batch.  Equal to the host path and to the run with the
    variable unset"""
    c = make()
    dup, cov = mode == "duplicates", mode == "coverage"
    assert max(len(sb) for sb in c.supers()) > 1
    got = check(pkg, monkeypatch, c, dup=dup, cov=cov)
    one = check(pkg, monkeypatch, c, fc.SUPER_1M, dup=dup, cov=cov)
    for k in got:
        assert _same(got[k], one[k]), (c.name, mode, k)
    if dup:
        assert make is not fc.sub_ragged or got["dup"][0]["flagged"] > 0


def _block_starts(bgzf):
    starts, p = [], 0
    while p < len(bgzf):
        starts.append(p)
        p += int.from_bytes(bgzf[p + 16:p + 18], "little") + 1
    return starts + [len(bgzf)]


def test_sub_batches_with_handoff(pkg, monkeypatch):
    """case 9: the ragged stream dealt to two engines in runs of 27 blocks (feed_handoff), every run more than one sub-batch"""
    c = fc.sub_ragged()
    records = b"".join(fc.records_of(c)[0])
    want = _host(pkg, c, records)
    _set_env(monkeypatch, c.env)
    bgzf, bounds = c.bgzf()
    at = _block_starts(bgzf)
    runs = list(range(0, len(at) - 1, 27)) + [len(at) - 1]
    assert len(runs) >= 4 and bounds[27] - bounds[0] > 131072 and c.head_len < bounds[1]
    engs = [_engine(pkg, c), _engine(pkg, c)]
    try:
        sink, prev = [], None
        for r, (b0, b1) in enumerate(zip(runs[:-1], runs[1:])):
            e = engs[r % 2]
            if prev is not None:
                prev.feed_handoff(e)
                sink.append(prev.finish_records().tobytes())   # the run's whole records; the one it ends inside goes with `e`
            e.submit_bgzf(np.frombuffer(bgzf[at[b0]:at[b1]], dtype=np.uint8), header_bytes=c.head_len if r == 0 else 0,
                          max_batch_inflated=c.max_batch)
            prev = e
        flags = [e.feed_status()["flags"] for e in engs]
        sink.append(prev.finish_records().tobytes())
        tabs = [e.finish() for e in engs]
    finally:
        for e in engs:
            e.close()
    assert flags == [0, 0]
    assert b"".join(sink) == records
    assert sum(t.stats["records"] for t in tabs) == c.n_records and min(t.stats["records"] for t in tabs) > 0
    for k in ("fwd", "rev", "k5", "k3"):
        assert np.array_equal(sum(getattr(t, k) for t in tabs), want[k]), k

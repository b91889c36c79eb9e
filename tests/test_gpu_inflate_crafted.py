"""The device inflate paths (csrc/inflate_kernels.h: in place, one wait per step with and without pieces;
csrc/inflate_wave.h: wave per block) on deflate streams zlib's compressor never writes, and on malformed ones, one
defect at a time: tests/deflate_craft_lib.py builds both corpora, tests/test_deflate_craft_host.py holds them to zlib.
Oracle: the writer's own LZ77 replay of its token lists (== zlib's output, asserted there).  All comparisons are exact."""
import struct
import zlib
from pathlib import Path

import numpy as np
import pytest

import deflate_craft_lib as dc
import pssbam_testlib as tl
from test_gpu_inflate import _bam_header_bytes, _contigs_of, inflate_loop, pkg  # noqa: F401  (the four-path fixture, autouse)

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden"
INF_BAD_CRC, INF_RETRY = 8, 100


def _first_difference(names, wants, got):
    o = 0
    for name, want in zip(names, wants):
        part = got[o:o + len(want)]
        if part != want:
            at = next((i for i, (a, b) in enumerate(zip(part, want)) if a != b), min(len(part), len(want)))
            return f"case {name}: first wrong byte at {at} of {len(want)} (got {part[at:at + 8].hex()}, want {want[at:at + 8].hex()})"
        o += len(want)
    return None


def test_valid_corpus_in_one_call(pkg):
    """Every valid case as one BGZF block of one buffer.  That this bites was tried once on a scratch build with one
    change per path, each of which keeps every access where it was and only makes a copy read bytes not yet written:
    seq_piece_of() returning 32 for every distance (wave per block: first failing case all_286_and_30_symbols), the
    in-place loop's `dist >= 8u` as `>= 7u` (in place: all_286_and_30_symbols), `pcap = INF_PIECE` without the min
    with the distance (one wait per step: dist_codes_9_to_15_bits), the deferred loop's `dist >= 64u` as `>= 63u`
    (whole copies: all_286_and_30_symbols) -- each flagged by the CRC kernel, status 8."""
    cases = dc.valid_cases()
    names, wants = [c[0] for c in cases], [c[2] for c in cases]
    buf = b"".join(dc.bgzf_frame(p, w) for _, p, w in cases) + tl.BGZF_EOF
    res = pkg.bgzf_inflate(np.frombuffer(buf, dtype=np.uint8))
    assert res["bad_block"] is None, f"case {names[res['bad_block']]} (block {res['bad_block']}) refused with status {res['bad_status']}"
    assert res["n_blocks"] == len(cases) + 1
    got = res["data"].tobytes()
    assert len(got) == sum(map(len, wants))
    assert got == b"".join(wants), _first_difference(names, wants, got)


@pytest.mark.parametrize("inflate_loop", ["wave-per-block"], indirect=True)     # (the hand-back is the wave path's alone)
def test_arena_cases_are_handed_back_and_retried(pkg, monkeypatch):
    """the two cases with more sequences than seq_cap_of(isize): without the second chance (PSSBAM_INFLATE_WAVE=2) the
    wave path leaves them in state INF_RETRY -- the corpus does reach the hand-back; with it (=1) the lane-per-block
    kernel behind it inflates them"""
    cases = {c[0]: c for c in dc.valid_cases()}
    good = cases["match_grid_dynamic"]
    for name in dc.ARENA_CASES:
        blocks = [good, cases[name], good]
        buf = np.frombuffer(b"".join(dc.bgzf_frame(p, w) for _, p, w in blocks) + tl.BGZF_EOF, dtype=np.uint8)
        monkeypatch.setenv("PSSBAM_INFLATE_WAVE", "2")
        res = pkg.bgzf_inflate(buf)
        assert (res["bad_block"], res["bad_status"]) == (1, INF_RETRY), (name, res["bad_block"], res["bad_status"])
        monkeypatch.setenv("PSSBAM_INFLATE_WAVE", "1")
        res = pkg.bgzf_inflate(buf)
        assert res["bad_block"] is None, (name, res["bad_block"], res["bad_status"])
        assert res["data"].tobytes() == b"".join(w for _, _, w in blocks), name


def test_invalid_corpus_is_refused_by_the_decoders(pkg):
    """The malformed block sits between good ones and is never the buffer's first: a decoder that followed a distance
    too far back, or wrote past ISIZE, would read / write its neighbours' bytes inside the allocation and come back
    with status 0 -- which is what is asserted against, with the CRC check off (the decoders themselves must refuse)
    and on.  The good blocks' bytes are intact either way."""
    rng = np.random.default_rng(77)
    good = []
    for n in (300, 1, 4000, 65):
        data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
        good.append((dc.bgzf_frame(dc.Deflate().fixed(list(data), final=True).payload(), data), data))
    for c in dc.invalid_case_objects():
        name, isize, lenient = c.name, c.isize, c.name in dc.LENIENT
        crc = zlib.crc32(c.intended if lenient else bytes(isize)) & 0xFFFFFFFF
        for check_crc, crc_field in ((False, crc), (True, crc), (True, crc ^ 0x5A5A)):
            bad = dc.bgzf_frame(c.payload, isize=isize, crc=crc_field)
            buf = good[0][0] + good[1][0] + bad + good[2][0] + good[3][0] + tl.BGZF_EOF
            res = pkg.bgzf_inflate(np.frombuffer(buf, dtype=np.uint8), check_crc=check_crc)
            got, o = res["data"].tobytes(), 0
            assert res["n_blocks"] == 6 and len(got) == sum(len(d) for _, d in good) + isize, name
            for k, (_, d) in enumerate(good):
                o += isize if k == 2 else 0
                assert got[o:o + len(d)] == d, (name, check_crc, "good block damaged", k)
                o += len(d)
            if lenient:
                # dc.LENIENT: an incomplete code whose missing codes never occur.  The decoders refuse over-subscribed
                # sets (the only ones that lead a canonical decoder out of its tables) and any bit pattern that falls
                # into the hole (incomplete_*_hole_used, strict below), not the incomplete set as such, as zlib does.
                # What guards this case is the CRC check, so only its outcome is pinned: under the CRC of what the
                # writer meant the block is refused or holds exactly those bytes, under any other CRC it is refused.
                if check_crc and crc_field == crc:
                    at = len(good[0][1]) + len(good[1][1])
                    assert res["bad_block"] == 2 or (res["bad_block"] is None and got[at:at + isize] == c.intended), (name, res["bad_block"], res["bad_status"])
                elif check_crc:
                    assert res["bad_block"] == 2 and res["bad_status"] != 0, (name, res["bad_block"], res["bad_status"])
                continue
            assert res["bad_block"] == 2 and res["bad_status"] != 0, (name, check_crc, res["bad_block"], res["bad_status"])
            if not check_crc:
                assert res["bad_status"] != INF_BAD_CRC


def _bam_header(data: bytes):
    """(inflated bytes in front of the first alignment record, the reference names) of a BAM's inflated bytes"""
    o = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref, o, names = struct.unpack_from("<i", data, o)[0], o + 4, []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", data, o)[0]
        names.append(data[o + 4:o + 4 + l_name - 1].decode())
        o += 4 + l_name + 4
    return o, names


def test_crafted_bam_through_the_engine_feed(pkg):
    """setA.bam re-compressed by the crafted writer (comb codes up to 15 bits, 4 KiB blocks that cut through records)
    through Engine.submit_bgzf -- the feed's own inflate launch and the record chain over these blocks: same tables and
    status tallies as submit() on the raw records"""
    raw = dc.crafted_setA_bgzf()
    data = dc.record_stream()
    hb, refs = _bam_header(data)
    assert 0 < hb < len(data) and hb == _bam_header_bytes(raw)
    contigs = _contigs_of(GOLD / "setA.fa")
    pss, kmer = dict(region_len=15), dict(klen=4)
    want = None
    for max_batch in ("host path", "default batch", 70000):
        eng = pkg.Engine(pss=pss, kmer=kmer)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references(refs)
        if max_batch == "host path":
            eng.submit(np.frombuffer(data[hb:], dtype=np.uint8))
        else:
            kw = {} if max_batch == "default batch" else dict(max_batch_inflated=max_batch)
            eng.submit_bgzf(np.frombuffer(raw, dtype=np.uint8), header_bytes=hb, **kw)
            assert eng.feed_status()["flags"] == 0, (max_batch, eng.feed_status())
        got = eng.finish()
        eng.close()
        if want is None:
            want = got
            assert got.stats["records"] > 100 and got.fwd.sum() > 0
            continue
        assert np.array_equal(got.fwd, want.fwd) and np.array_equal(got.rev, want.rev), max_batch
        assert np.array_equal(got.k5, want.k5) and np.array_equal(got.k3, want.k3), max_batch
        a, b = dict(got.stats), dict(want.stats)
        a.pop("slow_path"), b.pop("slow_path")
        assert a == b, (max_batch, got.stats, want.stats)

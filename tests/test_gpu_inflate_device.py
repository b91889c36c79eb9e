"""pssbam_bgzf_inflate_device (include/pssbam_hip.h), the public entry point that inflates on a CALLER's device buffers,
with the caller's block table, on the caller's stream -- and the only caller of launch_inflate (csrc/bgzf_api.h) that
forces the in-place data loop and passes no wave buffers.  What the header promises is checked here on buffers without
the slack the project's own callers have: every block at its own out_off & 15, 1..40 guard bytes between the blocks, the
blocks placed in reversed order, a canary byte everywhere else (tests/bgzf_device_lib.py builds all of it,
tests/test_bgzf_device_host.py proves the fixtures on the CPU).  Reference: zlib.  All comparisons are exact.

That this bites was tried once on scratch builds with one change each: store_tail16 as a full 16-byte store in the in-place
loop's far-match path (the parity tests fail on a guard byte), the CRC kernels' `b.status != INF_OK` skip removed (the
bad-descriptor and check_crc tests fail: statuses relabelled 8), their bi stride doubled (the large table fails).  The
`isize > 65536u` descriptor check was only read, not run without: the isize = 65537 entry would be inflated, status 6 and
bytes in a range that must keep the canary."""
import struct
import zlib

import numpy as np
import pytest

import bgzf_device_lib as bd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return bd.load_pkg()


def _kinds_corpus():
    """the payload kinds of tests/test_gpu_inflate.py (its helpers, not a copy of its data): stored, fixed, dynamic and
    multi-deflate-block BGZF blocks, and what zlib inflates them to"""
    from test_gpu_inflate import _bgzf, _payloads
    blocks, want = [], []
    for data in _payloads(np.random.default_rng(11)):
        for level, strategy, split in ((0, zlib.Z_DEFAULT_STRATEGY, None), (1, zlib.Z_DEFAULT_STRATEGY, None),
                                       (6, zlib.Z_DEFAULT_STRATEGY, None), (9, zlib.Z_DEFAULT_STRATEGY, None),
                                       (6, zlib.Z_FIXED, None), (6, zlib.Z_HUFFMAN_ONLY, None), (6, zlib.Z_RLE, None),
                                       (6, zlib.Z_DEFAULT_STRATEGY, (len(data) // 3, len(data) // 3)),
                                       (1, zlib.Z_FIXED, (len(data) // 2,))):
            if level == 0 and len(data) > 65000:
                continue     # a stored 64 KiB payload plus its framing exceeds the BGZF block size
            b = _bgzf(data, level, strategy, split)
            o, n, _, _ = bd.parse_block(b)
            blocks.append(b)
            want.append(zlib.decompress(b[o:o + n], -15))
            assert want[-1] == data
    assert {(b[18] >> 1) & 3 for b in blocks if len(b) > 26} == {0, 1, 2}
    return blocks, want


@pytest.fixture(scope="module")
def corpus():
    blocks, want = _kinds_corpus()
    n = len(blocks)
    aligns, gaps = [(7 * i + 1) % 16 for i in range(n)], [1 + (i % 40) for i in range(n)]
    assert set(aligns) == set(range(16)) and set(gaps) == set(range(1, 41))
    comp, comp_bytes, tab, out_bytes = bd.table_of(blocks, aligns, gaps)
    return comp, comp_bytes, tab, out_bytes, want, bd.expected_output(tab, want, out_bytes)


@pytest.mark.parametrize("env", [None, ("PSSBAM_INFLATE_LOOP", "1"), ("PSSBAM_INFLATE_WAVE", "1")], ids=["plain", "loop-1", "wave-1"])
def test_parity_on_caller_buffers(pkg, corpus, monkeypatch, env):
    """every block's bytes are zlib's, every status is 0 and no byte outside the blocks' ranges -- in front of the first, in
    the 1..40 byte gaps, behind the last -- has changed; the same with PSSBAM_INFLATE_LOOP=1 and PSSBAM_INFLATE_WAVE=1 in the
    environment, which a caller's buffers must not feel (they have no slack for the other data loops)"""
    for k in ("PSSBAM_INFLATE_LOOP", "PSSBAM_INFLATE_WAVE", "PSSBAM_INFLATE_PIECES"):
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(*env)
    comp, comp_bytes, tab, out_bytes, want, want_out = corpus
    for check_crc in (0, 1):
        rc, status, out = bd.run_device(pkg, comp, comp_bytes, tab, out_bytes, check_crc)
        assert rc == bd.PSSBAM_OK
        bad = np.flatnonzero(status)
        assert bad.size == 0, f"block {int(bad[0])} ({int(tab['isize'][bad[0]])} bytes): status {int(status[bad[0]])}"
        assert bd.first_difference(out, want_out, tab) is None, bd.first_difference(out, want_out, tab)


def _tail_tables():
    """tables whose last payload ends exactly at comp_bytes, one per comp_bytes % 4 and per kind of last block (dynamic,
    stored, fixed): the residue is picked by the last block's payload length"""
    rng = np.random.default_rng(21)
    front = [bd.payload_bytes(rng, 3000), bytes(rng.integers(0, 256, 700, dtype=np.uint8)), bd.payload_bytes(rng, 1)]
    front_blocks = [bd.block(front[0], 6), bd.block(front[1], 0), bd.block(front[2], 1)]
    tables = []
    for kind, (level, strategy) in enumerate(((1, zlib.Z_DEFAULT_STRATEGY), (0, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED))):
        found = {}
        for n in range(400, 480):
            data = bd.payload_bytes(rng, n)
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            payload = co.compress(data) + co.flush()
            if (payload[0] >> 1) & 3 != (2, 0, 1)[kind]:
                continue
            last = bd.BGZF_HEAD + struct.pack("<H", len(payload) + 25) + payload + struct.pack("<II", zlib.crc32(data), n)
            comp, comp_bytes, tab, out_bytes = bd.table_of(front_blocks + [last], [3, 9, 0, 14], 2, cut_last_trailer=True)
            if comp_bytes % 4 not in found:
                found[comp_bytes % 4] = (comp, comp_bytes, tab, out_bytes, front + [data])
            if len(found) == 4:
                break
        assert sorted(found) == [0, 1, 2, 3], (kind, sorted(found))
        tables += [found[r] for r in range(4)]
    # ... and one whose whole compressed buffer is shorter than 64 bytes
    tiny = [b"A", b"ACGTACGT"]
    comp, comp_bytes, tab, out_bytes = bd.table_of([bd.block(d, 1) for d in tiny], [15, 5], 1, cut_last_trailer=True)
    assert comp_bytes < 64
    tables.append((comp, comp_bytes, tab, out_bytes, tiny))
    return tables


def test_nothing_depends_on_the_bytes_behind_comp_bytes(pkg):
    """the same table with the 64 bytes behind comp_bytes holding 0x00 and then 0xFF: statuses and the whole output buffer are
    identical and zlib's, for comp_bytes % 4 = 0..3 with the last payload ending exactly at comp_bytes"""
    tables = _tail_tables()
    assert {t[1] % 4 for t in tables[:-1]} == {0, 1, 2, 3}
    for comp, comp_bytes, tab, out_bytes, datas in tables:
        assert int(tab["in_off"][-1]) + int(tab["in_len"][-1]) == comp_bytes
        want_out = bd.expected_output(tab, datas, out_bytes)
        runs = []
        for fill in (0x00, 0xFF):
            rc, status, out = bd.run_device(pkg, comp, comp_bytes, tab, out_bytes, 1, tail_fill=fill)
            assert rc == bd.PSSBAM_OK and not status.any(), (comp_bytes, fill, status.tolist())
            assert bd.first_difference(out, want_out, tab) is None, (comp_bytes, fill, bd.first_difference(out, want_out, tab))
            runs.append((status, out))
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def test_bad_descriptors_get_their_status_and_are_not_touched(pkg):
    """a table that mixes good blocks with descriptors that cannot be: isize 65537, in_off behind comp_bytes, in_off + in_len
    behind comp_bytes, in_off = 2^40 -- status 1 each, their output ranges still the canary -- and an in_len one byte short,
    whose stream is truncated (a decoder status, 1..7; what it wrote stays inside its own range).  Every good block is
    inflated correctly, with and without the CRC kernel behind (which must leave these statuses alone)."""
    rng = np.random.default_rng(31)
    datas = [bd.payload_bytes(rng, n) for n in (500, 17, 4000, 1, 300, 65536, 900, 64, 2049, 33, 700, 5)]
    blocks = [bd.block(d, 1 + i % 6) for i, d in enumerate(datas)]
    bad_at = {1: "isize", 4: "in_off", 6: "in_end", 8: "far", 10: "short"}
    sizes = [65537 if bad_at.get(i) == "isize" else len(d) for i, d in enumerate(datas)]
    comp, comp_bytes, tab, _ = bd.table_of(blocks, [(3 * i + 2) % 16 for i in range(len(blocks))], 1)
    lay, out_bytes = bd.layout(sizes, [(3 * i + 2) % 16 for i in range(len(blocks))], [1 + i for i in range(len(blocks))])
    tab["out_off"], tab["isize"] = lay["out_off"], lay["isize"]
    for i, what in bad_at.items():
        if what == "in_off":
            tab["in_off"][i] = comp_bytes + 1
        elif what == "in_end":
            tab["in_off"][i], tab["in_len"][i] = comp_bytes - 10, 11
        elif what == "far":
            tab["in_off"][i] = 1 << 40
        elif what == "short":
            tab["in_len"][i] -= 1
    want_out = bd.expected_output(tab, [None if i in bad_at else d for i, d in enumerate(datas)], out_bytes)
    s_at, s_len = int(tab["out_off"][10]), len(datas[10])
    for check_crc in (0, 1):
        rc, status, out = bd.run_device(pkg, comp, comp_bytes, tab, out_bytes, check_crc)
        assert rc == bd.PSSBAM_OK
        for i in range(len(blocks)):
            if bad_at.get(i) == "short":
                assert 1 <= status[i] <= 7, (check_crc, int(status[i]))
            else:
                assert status[i] == (bd.INF_BAD_BLOCK if i in bad_at else bd.INF_OK), (check_crc, i, bad_at.get(i), int(status[i]))
        want = want_out.copy()
        want[s_at:s_at + s_len] = out[s_at:s_at + s_len]          # (the truncated block's own range: not pinned)
        assert bd.first_difference(out, want, tab) is None, (check_crc, bd.first_difference(out, want, tab))


def test_check_crc_flags_wrong_bytes_and_leaves_decoder_statuses(pkg):
    """a block that inflates cleanly to bytes its trailer does not describe: status 0 and those bytes without the CRC kernel,
    exactly 8 with it.  Blocks the DECODER refuses (a reserved block type, an ISIZE above and below what the stream holds)
    keep their status 1..7 under check_crc = 1: the CRC kernel skips what is not OK and relabels nothing."""
    rng = np.random.default_rng(41)
    data = [bd.payload_bytes(rng, n) for n in (1200, 1200, 800, 640, 640, 77)]
    wrong = bd.change_byte(data[1], 600)
    reserved = bd.BGZF_HEAD + struct.pack("<H", 25 + 1) + b"\x07" + struct.pack("<II", 0x12345678, 800)    # BFINAL, BTYPE = 3
    longer, shorter = bytearray(bd.block(data[3], 6)), bytearray(bd.block(data[4], 6))
    struct.pack_into("<I", longer, len(longer) - 4, 645)
    struct.pack_into("<I", shorter, len(shorter) - 4, 635)
    blocks = [bd.block(data[0], 6), bd.block(wrong, 6, trailer_of=data[1]), reserved, bytes(longer), bytes(shorter), bd.block(data[5], 1)]
    comp, comp_bytes, tab, out_bytes = bd.table_of(blocks, [4, 11, 0, 7, 13, 2], 1)
    pinned = [data[0], wrong, None, None, None, data[5]]
    want_out = bd.expected_output(tab, pinned, out_bytes)
    seen = {}
    for check_crc in (0, 1):
        rc, status, out = bd.run_device(pkg, comp, comp_bytes, tab, out_bytes, check_crc)
        assert rc == bd.PSSBAM_OK
        assert status[0] == 0 and status[5] == 0
        assert status[1] == (bd.INF_BAD_CRC if check_crc else bd.INF_OK), (check_crc, int(status[1]))
        assert all(1 <= status[i] <= 7 for i in (2, 3, 4)), (check_crc, status.tolist())
        seen[check_crc] = status[2:5].tolist()
        want = want_out.copy()
        for i in (2, 3, 4):                                      # (a refused block's own range is not pinned; everything around it is)
            o, n = int(tab["out_off"][i]), int(tab["isize"][i])
            want[o:o + n] = out[o:o + n]
        assert bd.first_difference(out, want, tab) is None, (check_crc, bd.first_difference(out, want, tab))
    assert seen[0] == seen[1] and seen[0][0] == bd.INF_BAD_BLOCK, seen


@pytest.fixture(scope="module")
def large_table():
    """more than two grid passes of the inflate kernel (CUs * 4 waves * 64 lanes per pass) and many of either CRC kernel:
    tiny blocks, every 7th with a trailer that describes other bytes"""
    import torch
    n = 2 * (torch.cuda.get_device_properties(0).multi_processor_count * 4 * 64) + 77
    rng = np.random.default_rng(51)
    lens = rng.integers(8, 25, n).tolist()
    raw = bd.payload_bytes(rng, sum(lens))
    blocks, datas, o = [], [], 0
    for i, ln in enumerate(lens):
        d = raw[o:o + ln]
        o += ln
        if i % 7 == 0:
            datas.append(bd.change_byte(d, i % ln))
            blocks.append(bd.block(datas[-1], 1, trailer_of=d))
        else:
            datas.append(d)
            blocks.append(bd.block(d, 1))
    comp, comp_bytes, tab, out_bytes = bd.table_of(blocks, [i % 16 for i in range(n)], 1)
    want_status = np.where(np.arange(n) % 7 == 0, bd.INF_BAD_CRC, bd.INF_OK).astype(np.uint32)
    return comp, comp_bytes, tab, out_bytes, want_status, bd.expected_output(tab, datas, out_bytes)


def test_every_block_of_a_large_table_is_visited(pkg, large_table):
    """statuses are exactly 8 on every 7th block and 0 elsewhere, the output is zlib's: a block the inflate kernel's
    grid-stride loop skipped would keep the canary, one a CRC kernel skipped would keep status 0"""
    comp, comp_bytes, tab, out_bytes, want_status, want_out = large_table
    assert len(tab) > 2 * 64 * 4 * 64 and out_bytes < 16 << 20
    rc, status, out = bd.run_device(pkg, comp, comp_bytes, tab, out_bytes, 1)
    assert rc == bd.PSSBAM_OK
    wrong = np.flatnonzero(status != want_status)
    assert wrong.size == 0, f"{wrong.size} of {len(tab)} blocks, first {int(wrong[0])}: status {int(status[wrong[0]])}, expected {int(want_status[wrong[0]])}"
    assert bd.first_difference(out, want_out, tab) is None, bd.first_difference(out, want_out, tab)


def test_arguments_and_streams(pkg):
    rng = np.random.default_rng(61)
    datas = [bd.payload_bytes(rng, n) for n in (100, 5000, 31)]
    comp, comp_bytes, tab, out_bytes = bd.table_of([bd.block(d, 6) for d in datas], [1, 2, 3], 5)
    want_out = bd.expected_output(tab, datas, out_bytes)
    canary = np.full(out_bytes, bd.CANARY, dtype=np.uint8)
    d_comp, d_blocks, d_out = bd.upload(comp, comp_bytes, tab, out_bytes)
    # no blocks: OK, and nothing is touched (not even looked at: the pointers may be anything)
    assert bd.call(pkg, d_comp, comp_bytes, d_blocks, 0, d_out, 1) == bd.PSSBAM_OK
    assert bd.call(pkg, d_comp, comp_bytes, d_blocks, 0, d_out, 1, null="out") == bd.PSSBAM_OK
    assert np.array_equal(d_out.cpu().numpy()[:out_bytes], canary)
    for null in ("comp", "blocks", "out"):
        assert bd.call(pkg, d_comp, comp_bytes, d_blocks, len(tab), d_out, 1, null=null) == bd.PSSBAM_EINVAL, null
    # d_comp must be 4-byte aligned
    assert bd.call(pkg, d_comp, comp_bytes, d_blocks, len(tab), d_out, 1, comp_shift=1) == bd.PSSBAM_EINVAL
    assert b"aligned" in pkg.hip_lib().pssbam_last_error()
    assert np.array_equal(d_out.cpu().numpy()[:out_bytes], canary)
    assert not d_blocks.cpu().numpy().view(bd.BLOCK_DTYPE)["status"].any()
    # stream 0 and a stream of the caller's
    for own_stream in (False, True):
        rc, status, out = bd.run_device(pkg, comp, comp_bytes, tab, out_bytes, 1, own_stream=own_stream)
        assert rc == bd.PSSBAM_OK and not status.any(), (own_stream, status.tolist())
        assert bd.first_difference(out, want_out, tab) is None, (own_stream, bd.first_difference(out, want_out, tab))

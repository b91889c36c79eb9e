"""tests/bgzf_device_lib.py proved on the CPU, so that a failure of tests/test_gpu_inflate_device.py or
tests/test_gpu_crc_edges.py points at the kernels and not at the fixtures: the blocks scan (pssbam_bgzf_scan, host code) and
inflate with zlib to what they claim, a trailer_of block's CRC field is NOT that of its bytes, layout() keeps its promises for
all sixteen alignments, changed_positions() reaches every arm of the CRC kernels, and EDGE_SIZES is pinned value by value.
Needs no GPU."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import __graft_entry__ as ge
import bgzf_device_lib as bd


@pytest.fixture(scope="module")
def scan():
    L = ge.load_pkg().hip_lib()
    L.pssbam_bgzf_scan.restype = C.c_int64
    L.pssbam_bgzf_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]

    def run(raw: bytes):
        buf = np.frombuffer(raw, dtype=np.uint8)
        consumed = C.c_uint64()
        n = L.pssbam_bgzf_scan(buf.ctypes.data, buf.size, None, 0, C.byref(consumed), None)
        assert n >= 0 and consumed.value == len(raw)
        tab = np.zeros(n, dtype=bd.BLOCK_DTYPE)
        assert L.pssbam_bgzf_scan(buf.ctypes.data, buf.size, tab.ctypes.data, n, None, None) == n
        return tab
    return run


@pytest.fixture(scope="module")
def matrix_cases():
    return bd.crc_matrix_cases()


def test_edge_sizes_are_pinned():
    """every value by name: the list cannot be thinned without this test saying so"""
    named = ([0, 1, 2, 15, 16, 17, 31, 32, 33] + list(range(1007, 1042)) + [2047, 2048, 2049]
             + [8175, 8176, 8191, 8192, 8193, 8207, 8208, 8209] + [16383, 16384, 16385] + [64511, 64512, 64513]
             + [65519, 65520, 65535, 65536])
    assert len(named) == 65
    for T in named:
        assert T in bd.EDGE_SIZES, T
    for T in (1007, 1008, 1023, 1024, 1025, 1040, 1041, 16 * 63, 16 * 64, 16 * 65, 8 * 64 * 16, 63 * 1024 + 1, 65536):
        assert T in bd.EDGE_SIZES, T
    assert len(set(bd.EDGE_SIZES)) == len(bd.EDGE_SIZES) and max(bd.EDGE_SIZES) == 65536
    for T in bd.EDGE_SIZES:
        assert bd.matrix_alignments(T) == (list(range(16)) if T <= 2049 else [0, 1, 8, 15]), T


def test_blocks_scan_and_inflate_to_their_data(scan):
    rng = np.random.default_rng(1)
    datas, blocks = [], []
    for T in bd.EDGE_SIZES:
        for level in (1, 6) if T not in (65535, 65536) else (1,):
            datas.append(bd.payload_bytes(rng, T))
            blocks.append(bd.block(datas[-1], level))
    assert all(set(d) <= set(b"ACGT") for d in datas)
    assert max(len(b) for b in blocks) <= 65536 and len(bd.block(bd.payload_bytes(rng, 65536), 1)) < 40000
    raw = b"".join(blocks)
    tab = scan(raw)
    assert len(tab) == len(blocks)
    off = 0
    for b, d, row in zip(blocks, datas, tab):
        o, n, crc, isize = bd.parse_block(b)
        assert (int(row["in_off"]), int(row["in_len"]), int(row["crc"]), int(row["isize"])) == (off + o, n, crc, isize)
        assert zlib.decompress(raw[off + o:off + o + n], -15) == d
        assert isize == len(d) and crc == zlib.crc32(d) & 0xFFFFFFFF
        off += len(b)
    # table_of() says what the scan says, but for out_off (the caller's) -- also with the last trailer cut off
    comp, comp_bytes, mine, _ = bd.table_of(blocks, [0] * len(blocks), 1)
    for f in ("in_off", "in_len", "isize", "crc"):
        assert np.array_equal(mine[f], tab[f]), f
    assert comp_bytes == len(raw) and comp.tobytes() == raw
    _, cut_bytes, cut, _ = bd.table_of(blocks, [0] * len(blocks), 1, cut_last_trailer=True)
    assert cut_bytes == len(raw) - 8 == int(cut["in_off"][-1]) + int(cut["in_len"][-1])


def test_trailer_of_blocks_inflate_cleanly_to_other_bytes(scan):
    rng = np.random.default_rng(2)
    for T in (1, 2, 17, 1024, 8193, 65536):
        data = bd.payload_bytes(rng, T)
        for p in bd.changed_positions(T, 3):
            other = bd.change_byte(data, p)
            assert len(other) == T and [i for i in range(T) if other[i] != data[i]] == [p]
            b = bd.block(other, 1, trailer_of=data)
            row = scan(b)[0]
            got = zlib.decompress(b[int(row["in_off"]):int(row["in_off"]) + int(row["in_len"])], -15)      # no error: the stream is sound
            assert got == other and int(row["isize"]) == T
            assert int(row["crc"]) == zlib.crc32(data) & 0xFFFFFFFF != zlib.crc32(got) & 0xFFFFFFFF
    with pytest.raises(AssertionError):
        bd.block(b"ACGT", 1, trailer_of=b"ACG")
    empty = bd.block(b"", 1)
    assert struct.unpack_from("<II", empty, len(empty) - 8) == (0, 0) and zlib.crc32(b"") == 0
    assert struct.unpack_from("<II", bd.block(b"", 1, crc=7), len(empty) - 8) == (7, 0)


def test_matrix_cases_are_what_they_claim(matrix_cases):
    """every block of the CRC matrix: sound stream, ISIZE right, CRC field right exactly when the wanted status is 0"""
    seen = set()
    total = 0
    for T, a, p, b, data, want in matrix_cases:
        o, n, crc, isize = bd.parse_block(b)
        assert zlib.decompress(b[o:o + n], -15) == data and isize == T == len(data)
        assert (crc == zlib.crc32(data) & 0xFFFFFFFF) == (want == bd.INF_OK), (T, a, p)
        assert want == (bd.INF_OK if p is None else bd.INF_BAD_CRC)
        seen.add((T, a, p))
        total += T
    for T in bd.EDGE_SIZES:
        for a in bd.matrix_alignments(T):
            assert (T, a, None) in seen
            for p in bd.changed_positions(T, a):
                assert (T, a, p) in seen, (T, a, p)
    assert all((0, a, "crc") in seen for a in range(16))
    assert len(seen) == len(matrix_cases) and total < 100 << 20


def test_layout_alignments_gaps_and_order():
    rng = np.random.default_rng(3)
    for gap in (1, 7, 16, 40, list(range(1, 41)) * 2):
        n = 80
        sizes = [int(x) for x in rng.integers(0, 300, n)]
        aligns = [(5 * i + 3) % 16 for i in range(n)]
        assert set(aligns) == set(range(16))
        gaps = [gap] * n if isinstance(gap, int) else gap
        tab, out_bytes = bd.layout(sizes, aligns, gap)
        assert tab.dtype == bd.BLOCK_DTYPE and tab.dtype.names == ("in_off", "in_len", "isize", "out_off", "crc", "status")
        off = tab["out_off"].astype(np.int64)
        assert np.array_equal(off & 15, aligns) and tab["isize"].tolist() == sizes
        assert np.all(np.diff(off) < 0)                       # reversed: not the file order
        end = 0                                               # what lies in front of block i: the buffer's start, then block i + 1
        for i in range(n - 1, -1, -1):
            g = int(off[i]) - end
            assert gaps[i] <= g < gaps[i] + 16, (i, g)        # the smallest gap >= the one asked for that gives the alignment
            end = int(off[i]) + sizes[i]
        assert out_bytes == end + gaps[0]
    tab, out_bytes = bd.layout([], [], 5)
    assert len(tab) == 0 and out_bytes == 0


def test_changed_positions_reach_every_arm():
    for T in bd.EDGE_SIZES:
        for a in range(16):
            pos = bd.changed_positions(T, a)
            assert pos == sorted(set(pos)) and all(0 <= p < T for p in pos), (T, a)
            if T <= 33:
                assert pos == list(range(T))
                continue
            assert len(pos) <= 15
            # the lines kernel's view of the block (csrc/inflate_kernels.h: head, n_full pieces of 16, tail)
            head = min((16 - a) & 15, T)
            n_full, tail = (T - head) >> 4, (T - head) & 15
            assert n_full >= 1
            if head:
                assert any(p < head for p in pos), (T, a)
            assert any(head <= p < head + 16 for p in pos), (T, a)
            last = head + 16 * (n_full - 1)
            assert any(last <= p < last + 16 for p in pos), (T, a)
            if tail:
                assert any(p >= head + 16 * n_full for p in pos), (T, a)
            if n_full > 64:                                    # a lane's second piece, and the last piece of its first round
                assert any(head + 16 * 64 <= p < head + 16 * 65 for p in pos) and any(head + 16 * 63 <= p < head + 16 * 64 for p in pos)
            if n_full > 512:                                   # the second loop trip, and the last piece of the first
                assert any(head + 16 * 512 <= p < head + 16 * 513 for p in pos) and any(head + 16 * 511 <= p < head + 16 * 512 for p in pos)
            # the chunk kernel's view: 1 KiB chunks counted from the block's end
            if T > 1024:
                assert T - 1025 in pos and T - 1024 in pos     # the last byte of one lane's chunk, the first of the next lane's
    assert bd.changed_positions(40) == bd.changed_positions(40, 0)


def test_expected_output_and_first_difference():
    tab, out_bytes = bd.layout([4, 0, 3], [1, 2, 3], 2)
    datas = [b"ACGT", b"", None]
    want = bd.expected_output(tab, datas, out_bytes)
    o = tab["out_off"].tolist()
    assert want[o[0]:o[0] + 4].tobytes() == b"ACGT" and int((want != bd.CANARY).sum()) == 4
    assert bd.first_difference(want.copy(), want, tab) is None
    got = want.copy()
    got[o[0] + 4] = 0
    assert "guard byte" in bd.first_difference(got, want, tab) and ", 0 bytes behind the end of block 0" in bd.first_difference(got, want, tab)
    got = want.copy()
    got[o[0] + 2] = 0
    assert "2 of block 0" in bd.first_difference(got, want, tab)

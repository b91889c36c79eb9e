"""Judges of BGZF output that own nothing of the code under test: a walker over the blocks of a buffer (Python's zlib inflates
and checksums) and the inputs of the deflate tests."""
import struct
import zlib

import numpy as np

PAYLOAD = 0xFF00                    # bytes of the stream per block of the device deflate (csrc/deflate_kernels.h DFL_PAYLOAD)
STORED_EXTRA = 5 + 26               # a stored block over its payload: 1 + LEN + NLEN, the 18-byte header, CRC-32 and ISIZE
EOF_BLOCK = bytes([0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def walk(data: bytes) -> list:
    """[(block bytes, payload)] of every BGZF block of data; every block is checked: magic, the BC subfield, BSIZE == block
    length - 1 <= 65535, one complete raw DEFLATE stream with nothing behind it, ISIZE <= 0xFF00, CRC-32 of the inflated bytes"""
    out, i = [], 0
    while i < len(data):
        assert len(data) - i >= 26, f"{len(data) - i} bytes behind the last block"
        assert data[i:i + 4] == b"\x1f\x8b\x08\x04", f"no gzip magic with FEXTRA at byte {i}"
        assert data[i + 10:i + 12] == b"\x06\x00" and data[i + 12:i + 16] == b"BC\x02\x00", f"no BC subfield at byte {i}"
        bsize = struct.unpack_from("<H", data, i + 16)[0]
        assert bsize <= 65535 and i + bsize + 1 <= len(data), "BSIZE does not frame the block"
        block = data[i:i + bsize + 1]
        z = zlib.decompressobj(-15)
        payload = z.decompress(block[18:-8])
        assert z.eof and not z.unused_data and not z.unconsumed_tail, "the DEFLATE stream does not end where the trailer starts"
        crc, isize = struct.unpack_from("<II", block, len(block) - 8)
        assert isize == len(payload) <= PAYLOAD, f"ISIZE {isize} for {len(payload)} bytes"
        assert crc == zlib.crc32(payload) & 0xFFFFFFFF, "CRC-32"
        out.append((block, payload))
        i += bsize + 1
    return out


def check_fixed_cut(data: bytes, raw: bytes) -> list:
    """the blocks of data are raw cut every PAYLOAD bytes: block k inflates to exactly raw[k * PAYLOAD : (k + 1) * PAYLOAD]; no
    block is larger than its stored form"""
    blocks = walk(data)
    assert len(blocks) == (len(raw) + PAYLOAD - 1) // PAYLOAD
    for k, (block, payload) in enumerate(blocks):
        assert payload == raw[k * PAYLOAD:(k + 1) * PAYLOAD], f"block {k} does not inflate to its payload"
        assert len(block) <= len(payload) + STORED_EXTRA, f"block {k}: {len(block)} bytes for {len(payload)}"
    return blocks


def btype(block: bytes) -> int:
    """BTYPE of the block's first DEFLATE block"""
    return (block[18] >> 1) & 3


def level1_size(raw: bytes) -> int:
    """what zlib level 1 makes of the same payloads, framed the same way"""
    total = 0
    for o in range(0, len(raw), PAYLOAD):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += 26 + len(c.compress(raw[o:o + PAYLOAD]) + c.flush())
    return total


def huffman_depth(counts) -> int:
    """the depth of an unrestricted Huffman code for the counts"""
    import heapq
    heap = [(int(c), 0) for c in counts if c]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def fibonacci_payload(seed: int = 11) -> bytes:
    """byte value 40 + k occurs fib(k) times (1, 1, 2, 3, ... the first 22): 46 367 bytes, shuffled"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    v = np.repeat(np.arange(40, 62, dtype=np.uint8), fib)
    np.random.default_rng(seed).shuffle(v)
    return v.tobytes()

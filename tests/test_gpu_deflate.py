"""BGZF deflate on the GPU (csrc/deflate_kernels.h) through pssbam_bgzf_deflate_host: every block is judged by Python's zlib
(deflate_lib.walk: framing, one complete raw DEFLATE stream, ISIZE, CRC-32) and must inflate to exactly the payload it stands
for -- the input cut every 0xFF00 bytes --; every output also goes back through the project's own device inflate with the
CRC check on.  Nothing on the expected side comes from the code under test.

The inputs are the smallest ones at which an encoder goes wrong: below the minimum match, runs (distance 1, lengths of 258,
the last byte inside a match), incompressible bytes (stored, and never larger than stored), matches only beyond the window,
a match at the window's edge, alphabets of one and of 256 equal symbols, counts whose Huffman code is deeper than 15, payloads
one byte around the cut, and streams of many blocks for the pack's scan and copies."""
import gzip
import zlib
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import deflate_lib as dl
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
P = dl.PAYLOAD


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


def golden_stream(base: str) -> bytes:
    return gzip.decompress((GOLD / f"{base}.bam").read_bytes())


def rnd(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def fuzz_stream(n_bytes: int, seed: int) -> bytes:
    """the record stream of tl.fuzz_dataset, n_bytes of it; a long one repeats its 2000 reads (the copies lie some 350 KB
    apart, far beyond the window, and at another offset in their blocks every time)"""
    contigs, refs, recs = tl.fuzz_dataset(seed, 2000, with_rg=True)
    raw = tl.raw_records(refs, recs).tobytes()
    assert len(raw) > 4 * P and len(raw) % P
    return (raw * -(-n_bytes // len(raw)))[:n_bytes]


def deflate(pkg, raw: bytes) -> bytes:
    res = pkg.bgzf_deflate(np.frombuffer(raw, dtype=np.uint8))
    data = res["data"].tobytes()
    blocks = dl.check_fixed_cut(data, raw)
    assert res["n_blocks"] == len(blocks)
    if raw:   # the project's own inflate, CRC-32 checked on the device
        back = pkg.bgzf_inflate(np.frombuffer(data, dtype=np.uint8), check_crc=True)
        assert back["bad_block"] is None and back["n_blocks"] == len(blocks) and back["data"].tobytes() == raw
    return data


def test_nothing_gives_no_block(pkg):
    res = pkg.bgzf_deflate(np.zeros(0, dtype=np.uint8))
    assert res["n_blocks"] == 0 and res["data"].size == 0


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_below_and_at_the_minimum_match(pkg, n):
    deflate(pkg, b"A" * n)
    deflate(pkg, bytes(range(65, 65 + n)))


def test_a_block_of_equal_bytes(pkg):
    data = deflate(pkg, b"\x07" * P)
    assert dl.btype(data) == 2 and len(data) < P // 16, len(data)   # (only an encoder that lost its matches misses this)


@pytest.mark.parametrize("n", [P - 1, P, P + 1])
def test_one_byte_around_the_cut(pkg, n):
    raw = golden_stream("setA")[:n]
    data = deflate(pkg, raw)
    assert len(dl.walk(data)) == (2 if n > P else 1) and len(data) < n


def test_random_bytes_come_out_stored(pkg):
    raw = rnd(P, 1)
    data = deflate(pkg, raw)
    assert dl.btype(data) == 0 and len(data) == P + dl.STORED_EXTRA <= 65536


def test_matches_beyond_the_window_are_not_taken(pkg):
    a = rnd(40000, 2)
    data = deflate(pkg, a + a[:P - 40000])       # the only matches sit at distance 40 000
    assert len(data) >= P                          # (nothing to gain: literals of random bytes)


def test_a_match_at_the_windows_edge(pkg):
    a = rnd(32768, 3)
    deflate(pkg, a + a[:P - 32768])              # distance 32 768 is legal: if it is emitted, zlib must read it back


def test_256_literals_of_equal_weight(pkg):
    order = np.random.default_rng(4).permutation(256).astype(np.uint8).tobytes()
    deflate(pkg, bytes(range(256)) + order)
    deflate(pkg, (bytes(range(256)) + order) * 3)   # (the same alphabet in a payload that is worth a dynamic block)


def test_one_distinct_literal(pkg):
    deflate(pkg, b"Q")                            # two symbols with the end of block, no match possible
    data = deflate(pkg, b"Q" * 300)               # one literal, one length, one distance code: HDIST's degenerate case
    assert len(data) < 300


def test_no_match_at_all_in_a_dynamic_block(pkg):
    """700 bytes of a skewed alphabet of 24 in which no three bytes in a row occur twice: worth a dynamic block (some 3.6
    bits a byte), and not one distance code in it"""
    rng, w = np.random.default_rng(5), 0.75 ** np.arange(24)
    out, seen = [], set()
    for _ in range(700):
        for _ in range(200):
            v = 65 + int(rng.choice(24, p=w / w.sum()))
            t = tuple(out[-2:] + [v])
            if len(t) < 3 or t not in seen:
                break
        seen.add(t)
        out.append(v)
    raw = bytes(out)
    assert len({raw[i:i + 3] for i in range(698)}) == 698
    data = deflate(pkg, raw)
    assert dl.btype(data) == 2 and len(data) < 700


def test_code_lengths_are_limited_to_15(pkg):
    raw = dl.fibonacci_payload()
    counts = np.bincount(np.frombuffer(raw, dtype=np.uint8))
    assert len(raw) == 46367 and dl.huffman_depth(counts) == 21   # an unrestricted code would be 21 deep
    data = deflate(pkg, raw)
    assert dl.btype(data) == 2 and len(data) < len(raw) // 2


@pytest.mark.parametrize("base,level1", [("setA", 0.59), ("setB", 0.62), ("setD", 0.55)])
def test_golden_streams(pkg, base, level1):
    raw = golden_stream(base)
    assert len(raw) == {"setA": 89777, "setB": 87500, "setD": 80475}[base]
    data = deflate(pkg, raw)
    z1 = dl.level1_size(raw)
    assert abs(z1 / len(raw) - level1) < 0.01
    print(f"{base}: {len(data)} bytes, {len(data) / len(raw):.3f} of raw, {len(data) / z1:.3f} of zlib level 1")
    assert len(dl.walk(data)) == 2 and len(data) < len(raw)


@pytest.mark.parametrize("n_blocks", [3, 70])
def test_streams_of_many_blocks(pkg, n_blocks):
    raw = fuzz_stream((n_blocks - 1) * P + 12345, seed=900 + n_blocks)
    data = deflate(pkg, raw)
    assert len(dl.walk(data)) == n_blocks and len(data) < len(raw)
    print(f"{n_blocks} blocks: {len(data) / len(raw):.3f} of raw, {len(data) / dl.level1_size(raw):.3f} of zlib level 1")


def test_the_bytes_do_not_depend_on_the_run(pkg):
    raw = golden_stream("setD") + b"\x00" * 5000 + rnd(3000, 6)
    outs = {pkg.bgzf_deflate(np.frombuffer(raw, dtype=np.uint8))["data"].tobytes() for _ in range(3)}
    assert len(outs) == 1
    dl.check_fixed_cut(outs.pop(), raw)
    # a payload's block does not depend on what else is in the launch: the first block alone
    alone = pkg.bgzf_deflate(np.frombuffer(raw[:P], dtype=np.uint8))["data"].tobytes()
    assert alone == dl.walk(deflate(pkg, raw))[0][0]

"""The three CRC-32 kernels behind launch_crc (csrc/bgzf_api.h, csrc/inflate_kernels.h) at the block sizes, alignments and
byte positions where their arithmetic changes branch -- and on the negative side: blocks that inflate CLEANLY to bytes
their trailer does not describe, which only the CRC check can refuse.  CRC-32 detects every error burst of up to 32 bits,
so each changed byte must be flagged: no case is left out.

* bgzf_crc_lines_kernel (the default)             the matrix of tests/bgzf_device_lib.py in this process;
* bgzf_crc_kernel<32> (PSSBAM_CRC_FORM=0)         the same matrix in a fresh child process (the switch is read once per
                                                  process), once more with one wave per workgroup (PSSBAM_CRC_WAVES=1);
* bgzf_crc_kernel<4> (beside the inflate kernel)  through the engine feed with PSSBAM_FEED_INFLATE_STREAMS=2.

The matrix: every T of EDGE_SIZES at out_off & 15 = 0..15 (T <= 2049) or {0, 1, 8, 15} (above), an intact block and one
block per entry of changed_positions(T, align); 47 MB of inflated data in one launch, so beyond the alignments named
nothing was dropped -- no size, no position.  Reference: zlib.  All comparisons are exact.

That this bites was tried once on scratch builds with one change each: n_full = (T - head + 15) >> 4 and xpow16[behind - 1]
in the lines kernel (test_lines_kernel_matrix fails), behind = (62 - lane) * CRC_CHUNK in the chunk kernel (both child
runs and the feed's good file fail), the bi stride of both kernels doubled (the lines matrix and both child runs fail)."""
import os

import numpy as np
import pytest

import bgzf_device_lib as bd
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu
FEED_BAD_BLOCK = 1
FEED_SIZES = [T for T in bd.EDGE_SIZES if T]
FEED_CYCLES = 3
N_GROUPS = 4


@pytest.fixture(scope="module")
def pkg():
    return bd.load_pkg()


def test_lines_kernel_matrix(pkg):
    """bgzf_crc_lines_kernel: intact blocks status 0, every changed block exactly 8, every block's bytes zlib's"""
    assert "PSSBAM_CRC_FORM" not in os.environ, "this process must run the default form of the CRC kernel"
    res = bd.crc_matrix(pkg)
    assert res["checked"] > 8000
    assert res["failures"] == [], res["failures"][:10]


@pytest.mark.parametrize("waves", [None, "1"], ids=["16-waves", "1-wave"])
def test_chunk_kernel_matrix_in_a_child(waves):
    """bgzf_crc_kernel<32>: the matrix through `python tests/bgzf_device_lib.py --crc-matrix` with PSSBAM_CRC_FORM=0; with
    PSSBAM_CRC_WAVES=1 the grid-stride loop does all the work with one wave per workgroup"""
    env = {"PSSBAM_CRC_FORM": "0"}
    if waves:
        env["PSSBAM_CRC_WAVES"] = waves
    rc, res, err = bd.crc_matrix_child(env)
    assert rc == 0 and res is not None, f"exit code {rc}\n{res}\n{err[-3000:]}"
    assert res["checked"] > 8000 and res["failures"] == [], f"{res['failures'][:10]}\n{err[-3000:]}"


# ---------------------------------------------------------------------------------------------------------------------
# bgzf_crc_kernel<4>: the engine feed with the inflate launches on streams of their own
# ---------------------------------------------------------------------------------------------------------------------
def _block(data: bytes) -> bytes:
    """(tl.bgzf_block stops at htslib's 0xFF00 bytes; the four edge sizes above it take the lib's builder: same framing)"""
    return tl.bgzf_block(data, 1) if len(data) <= 0xFF00 else bd.block(data, 1)


@pytest.fixture(scope="module")
def feed_set(pkg):
    """a record stream re-blocked into blocks whose sizes cycle through EDGE_SIZES (without 0).  out_off is the running sum
    and the list sums to a multiple of 16, so every cycle starts the list at another entry: a size then meets another
    alignment in every cycle.  Three cycles take 1.8 MB of records."""
    contigs, refs, recs = tl.fuzz_dataset(909, 14500)
    data = tl.bam_bytes(refs, recs)
    hb = len(tl.bam_bytes(refs, []))
    sizes = []
    for c in range(FEED_CYCLES):
        k = (21 * c) % len(FEED_SIZES)
        sizes += FEED_SIZES[k:] + FEED_SIZES[:k]
    assert sum(sizes) <= len(data) < sum(sizes) + (256 << 10), (sum(sizes), len(data))
    cuts = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    while cuts[-1] < len(data):                               # (what is left of the records: ordinary blocks)
        cuts.append(min(cuts[-1] + 0xFF00, len(data)))
    pieces = [data[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    aligns = {}
    for a, p in zip(cuts, pieces[:len(sizes)]):
        aligns.setdefault(len(p), set()).add(a & 15)
    assert all(len(v) >= 2 for T, v in aligns.items() if T % 16), aligns
    blocks = [_block(p) for p in pieces]
    pss = dict(region_len=15)
    eng = pkg.Engine(pss=pss)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([n for n, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    want = eng.finish()
    eng.close()
    assert want.stats["records"] == len(recs)
    return dict(contigs=contigs, refs=refs, hb=hb, pss=pss, pieces=pieces, blocks=blocks, cuts=cuts, want=want, n_sizes=len(sizes))


def _feed(pkg, fs, blocks):
    eng = pkg.Engine(pss=fs["pss"])
    eng.set_genome_arrays(tl.loaded_contigs(fs["contigs"]))
    eng.set_references([n for n, _ in fs["refs"]])
    eng.submit_bgzf(np.frombuffer(b"".join(blocks) + tl.BGZF_EOF, dtype=np.uint8), header_bytes=fs["hb"])
    st = eng.feed_status()
    got = eng.finish()
    eng.close()
    return got, st


@pytest.fixture
def two_streams(monkeypatch):
    monkeypatch.setenv("PSSBAM_FEED_INFLATE_STREAMS", "2")
    monkeypatch.setenv("PSSBAM_FEED_SUPER_BYTES", "1048576")   # several super-batches: the streams do take turns
    monkeypatch.delenv("PSSBAM_NO_CRC", raising=False)
    monkeypatch.delenv("PSSBAM_FEED_BIG_CRC", raising=False)


def test_small_table_kernel_passes_good_blocks_of_every_edge_size(pkg, feed_set, two_streams):
    """no flag, and tables and stats equal to submit() on the raw records"""
    got, st = _feed(pkg, feed_set, feed_set["blocks"])
    assert st["flags"] == 0, st
    want = feed_set["want"]
    assert np.array_equal(got.fwd, want.fwd) and np.array_equal(got.rev, want.rev)
    a, b = dict(got.stats), dict(want.stats)
    a.pop("slow_path"), b.pop("slow_path")
    assert a == b, (a, b)


@pytest.mark.parametrize("group", range(N_GROUPS))
def test_small_table_kernel_flags_wrong_bytes_at_every_edge_size(pkg, feed_set, two_streams, group):
    """per distinct edge size one block (of the second or third cycle: behind the BAM header) replaced by one that inflates
    cleanly to a changed first, last or (T - 1024)th byte under the old trailer: PSSBAM_FEED_BAD_BLOCK, one engine per case"""
    fs = feed_set
    n = len(FEED_SIZES)
    done = 0
    for j, T in enumerate(FEED_SIZES):
        if j % N_GROUPS != group:
            continue
        cycle = 1 + j % 2
        k = cycle * n + (j - 21 * cycle) % n                  # where size FEED_SIZES[j] sits in that cycle
        piece = fs["pieces"][k]
        assert len(piece) == T and fs["cuts"][k] > fs["hb"]
        at = [0, T - 1, T - 1024 if T >= 1024 else T // 2][j % 3]
        other = bd.change_byte(piece, at)
        blocks = list(fs["blocks"])
        blocks[k] = bd.block(other, 1, trailer_of=piece)
        _, st = _feed(pkg, fs, blocks)
        assert st["flags"] & FEED_BAD_BLOCK, (T, at, fs["cuts"][k] & 15, st)
        done += 1
    assert done >= n // N_GROUPS

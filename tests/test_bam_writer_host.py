"""CPU tests of the BAM writer (pss-bam_amd/host/bam_writer.c) through `hostcheck -a in.bam -w out.bam -z L -t T`, which
hands every batch of the reader to the writer, and of the command-line rules of pss-bam -O / -z (they end the command
before any work, so they need no GPU).

The file must hold the input's header and records byte for byte, in BGZF blocks of at most 0xFF00 payload bytes that
are cut where samtools cuts them -- the header in blocks of its own, a new block where the next record does not fit, a
record larger than a block across blocks -- and its bytes must not depend on the number of threads."""
import os
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import mismatch_lib as ml
import pssbam_testlib as tl

GOLD = Path(__file__).resolve().parent / "golden"
BLOCK_MAX = 0xFF00


@pytest.fixture(scope="module")
def bins():
    ge.build()
    b = ge.load_pkg().PKG_DIR / "bin"
    assert (b / "hostcheck").exists() and (b / "bam2sam").exists() and (b / "pss-bam").exists()
    return b


@pytest.fixture(scope="module")
def fuzz_bam(tmp_path_factory):
    """a fuzz_dataset BAM of a few hundred blocks' worth of batches: ragged input blocks, several output blocks"""
    d = tmp_path_factory.mktemp("writer_inputs")
    contigs, refs, recs = tl.fuzz_dataset(4402, 6000, with_rg=True)
    tl.write_bam(d / "fuzz.bam", refs, recs, level=1, rng=np.random.default_rng(5), block=6000)
    return d / "fuzz.bam"


def round_trip(bins, src, dst, level, threads, env=None):
    pr = subprocess.run([str(bins / "hostcheck"), "-a", str(src), "-w", str(dst), "-z", str(level), "-t", str(threads)],
                        capture_output=True, text=True, timeout=300, env={**os.environ, **(env or {})})
    assert pr.returncode == 0, pr.stderr
    assert not Path(str(dst) + ".tmp").exists()
    return Path(dst).read_bytes()


def blocks_of(data: bytes) -> list:
    """[(offset in the inflated stream, payload)] of every BGZF block; checks the framing of each"""
    out, i, at = [], 0, 0
    while i < len(data):
        assert data[i:i + 4] == b"\x1f\x8b\x08\x04" and data[i + 10:i + 16] == b"\x06\x00BC\x02\x00", "not a BGZF block in samtools layout"
        bsize = struct.unpack_from("<H", data, i + 16)[0] + 1
        assert bsize <= 65536 and i + bsize <= len(data), "BSIZE does not frame the block"
        payload = zlib.decompress(data[i + 18:i + bsize - 8], -15)
        crc, isize = struct.unpack_from("<II", data, i + bsize - 8)
        assert isize == len(payload) <= BLOCK_MAX and crc == zlib.crc32(payload) & 0xFFFFFFFF
        out.append((at, payload))
        at += len(payload)
        i += bsize
    assert i == len(data)
    return out


def header_bytes(raw: bytes) -> int:
    assert raw[:4] == b"BAM\1"
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    return o


def check_layout(data: bytes, want_raw: bytes):
    """the framing, the content, the EOF block, and where the blocks are cut"""
    assert data[-28:] == tl.BGZF_EOF
    blocks = blocks_of(data)
    assert blocks[-1][1] == b"" and all(p for _, p in blocks[:-1]), "one empty block, the last"
    assert b"".join(p for _, p in blocks) == want_raw == tl.bgzf_inflate(data)
    hb = header_bytes(want_raw)
    starts, o = set(), hb
    while o < len(want_raw):
        starts.add(o)
        o += 4 + struct.unpack_from("<I", want_raw, o)[0]
    assert o == len(want_raw)
    ends = sorted(starts | {len(want_raw)})
    for at, p in blocks[:-1]:
        if at < hb:
            assert at + len(p) <= hb, "the header has blocks of its own"
            continue
        if at in starts:
            # a block that starts with a record holds whole records, and the next record would not have fitted -- or the
            # record it starts with is larger than a block and fills it
            end = at + len(p)
            nxt = min(e for e in ends if e > at)
            if nxt - at > BLOCK_MAX:
                assert len(p) == BLOCK_MAX
            else:
                assert end in starts or end == len(want_raw)
                if end < len(want_raw):
                    assert min(e for e in ends if e > end) - at > BLOCK_MAX, "the block was closed although the next record fits"
        else:
            # the middle or the tail of a record larger than a block
            rec0 = max(s for s in starts if s < at)
            rec1 = min(e for e in ends if e > at)
            assert rec1 - rec0 > BLOCK_MAX and (at - rec0) % BLOCK_MAX == 0
    return blocks


@pytest.mark.parametrize("level", [0, 1, 6])
@pytest.mark.parametrize("src", ["setA", "setD", "fuzz"])
def test_round_trip(bins, fuzz_bam, tmp_path, src, level):
    path = fuzz_bam if src == "fuzz" else GOLD / f"{src}.bam"
    want_raw = tl.bgzf_inflate(path.read_bytes())
    one = round_trip(bins, path, tmp_path / "t1.bam", level, 1)
    eight = round_trip(bins, path, tmp_path / "t8.bam", level, 8)
    assert one == eight, "the file depends on the number of threads"
    # (small reader batches: many appends that end anywhere in a block -- the same file)
    assert round_trip(bins, path, tmp_path / "t3.bam", level, 3, {"PSSBAM_BATCH_BYTES": "70000"}) == one
    blocks = check_layout(one, want_raw)
    if src == "fuzz":
        assert len(blocks) > 8
    if level == 0:
        assert len(one) > len(want_raw)                   # stored blocks
    else:
        assert len(one) < len(want_raw)
    sam = lambda p: subprocess.run([str(bins / "bam2sam"), str(p)], capture_output=True, text=True, check=True).stdout
    text = sam(path)
    assert sam(tmp_path / "t8.bam") == text and text.count("\n") > 500


def test_levels_differ_and_are_what_zlib_gives(bins, fuzz_bam, tmp_path):
    outs = {z: round_trip(bins, fuzz_bam, tmp_path / f"z{z}.bam", z, 4) for z in (0, 1, 6, 9)}
    assert len({len(v) for v in outs.values()}) >= 3 and len(outs[6]) < len(outs[1]) < len(outs[0])
    for z, data in outs.items():       # every block is the raw deflate stream zlib writes for its payload at that level
        for _, p in blocks_of(data)[:3]:   # (level 0: how zlib cuts its stored blocks depends on how it is called)
            assert z == 0 or tl.bgzf_block(p, z) in data
    stored = blocks_of(outs[0])[1][1]      # level 0: stored blocks, the payload readable in the file
    assert stored[:4000] in outs[0]


def test_a_record_larger_than_a_block_spans_blocks(bins, tmp_path):
    text = ml.clean_contig(110000, seed=6)
    refs = [("long", len(text))]
    recs = [ml.read_on(text, 10 + j, 30, name=f"s{j}", rname="long") for j in range(5)]
    recs.insert(3, ml.read_on(text, 50, 100000, name="long_read", rname="long"))
    src = tmp_path / "in.bam"
    tl.write_bam(src, refs, recs)
    want_raw = tl.bgzf_inflate(src.read_bytes())
    for level in (0, 1):
        data = round_trip(bins, src, tmp_path / "out.bam", level, 8)
        assert data == round_trip(bins, src, tmp_path / "out1.bam", level, 1)
        blocks = check_layout(data, want_raw)
        sizes = [len(p) for _, p in blocks]
        assert sizes.count(BLOCK_MAX) == 2 and len(want_raw) > 150000
    # the block in front of the long record was closed at its start; the two short records behind it share the tail's block
    hb = header_bytes(want_raw)
    short = len(tl.bam_record(recs[0], {"long": 0}))
    assert [at for at, _ in blocks[:3]] == [0, hb, hb + 3 * short]


def test_no_records_gives_header_and_eof(bins, tmp_path):
    contigs, refs, _ = tl.fuzz_dataset(1, 10)
    src = tmp_path / "in.bam"
    tl.write_bam(src, refs, [])
    data = round_trip(bins, src, tmp_path / "out.bam", 6, 8)
    raw = tl.bgzf_inflate(src.read_bytes())
    assert header_bytes(raw) == len(raw)
    blocks = check_layout(data, raw)
    assert len(blocks) == 2 and data == tl.bgzf_block(raw, 6) + tl.BGZF_EOF


def test_unwritable_place_leaves_nothing(bins, tmp_path):
    pr = subprocess.run([str(bins / "hostcheck"), "-a", str(GOLD / "setA.bam"), "-w", str(tmp_path / "no" / "out.bam")], capture_output=True, text=True)
    assert pr.returncode == 1 and "cannot create" in pr.stderr and not list(tmp_path.iterdir())


# ---- pss-bam -O / -z: the command line's rules (no GPU: they end the command before any work) ---------------------------------

def pss(bins, tmp_path, *more, bam=GOLD / "setA.bam", env=None):
    return subprocess.run([str(bins / "pss-bam"), "-F", str(GOLD / "setA.fa"), "-B", str(bam), "-o", str(tmp_path / "out"), *more],
                          capture_output=True, text=True, timeout=60, env={**os.environ, **(env or {})})


@pytest.mark.parametrize("detach", ["0", "1"])
def test_cli_rejections(bins, tmp_path, detach):
    env = {"PSSBAM_DETACH_EXIT": detach}
    out = tmp_path / "o.bam"
    cases = {
        "sam": pss(bins, tmp_path, "-O", str(out), bam=GOLD / "setA.sam", env=env),
        "same": pss(bins, tmp_path, "-O", str(GOLD / "setA.bam"), env=env),
        "z10": pss(bins, tmp_path, "-O", str(out), "-z", "10", env=env),
        "z-1": pss(bins, tmp_path, "-O", str(out), "-z", "-1", env=env),
        "zx": pss(bins, tmp_path, "-O", str(out), "-z", "fast", env=env),
        "ngpu": pss(bins, tmp_path, "-O", str(out), env={**env, "PSSBAM_NGPU": "2"}),
        "z_alone": pss(bins, tmp_path, "-z", "3", env=env),
        "nowhere": pss(bins, tmp_path, "-O", str(tmp_path / "no" / "o.bam"), env=env),
    }
    for name, pr in cases.items():
        lines = pr.stderr.splitlines()
        assert pr.returncode == 1 and len(lines) == 1 and "Full command" not in pr.stderr and "Unknown option" not in pr.stderr, (name, pr.stderr)
    assert "SAM text" in cases["sam"].stderr and "must not name the input" in cases["same"].stderr and "0..9" in cases["z10"].stderr
    assert "cannot create" in cases["nowhere"].stderr and "0..9" in cases["z-1"].stderr and "0..9" in cases["zx"].stderr
    assert "PSSBAM_NGPU" in cases["ngpu"].stderr and "-O" in cases["z_alone"].stderr
    assert not list(tmp_path.iterdir()) and (GOLD / "setA.bam").stat().st_size > 40000


def test_same_file_by_another_name_is_rejected(bins, tmp_path):
    link = tmp_path / "alias.bam"
    link.symlink_to(GOLD / "setA.bam")
    pr = pss(bins, tmp_path, "-O", str(link), env={"PSSBAM_DETACH_EXIT": "0"})
    assert pr.returncode == 1 and pr.stderr.splitlines() == [f"-O must not name the input (-B {GOLD / 'setA.bam'})."] and link.is_symlink()


def test_usage_names_the_options(bins):
    pr = subprocess.run([str(bins / "pss-bam")], capture_output=True, text=True)
    assert pr.returncode == 1 and "-O <out.bam>" in pr.stderr and "-z <level>" in pr.stderr and "(default: 1)" in pr.stderr

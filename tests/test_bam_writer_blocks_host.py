"""CPU tests of bam_writer_append_blocks (pss-bam_amd/host/bam_writer.c), the writer's half of pss-bam -O ... -Z, through
`hostcheck -a in.bam -w out.bam -b`: the record stream is cut every 0xFF00 bytes there, each payload deflated with zlib, and
the finished blocks handed to the writer in uneven pieces.  The file must be the header's own blocks, then those blocks as
they are, then the EOF block; read back through the project's host reader it must hold the input's records; and a piece that
is not a whole number of blocks must fail the call and leave no file."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import deflate_lib as dl
import pssbam_testlib as tl
from test_bam_writer_host import header_bytes

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def bins():
    ge.build()
    b = ge.load_pkg().PKG_DIR / "bin"
    assert (b / "hostcheck").exists() and (b / "bam2sam").exists()
    return b


@pytest.fixture(scope="module")
def fuzz_bam(tmp_path_factory):
    """the input of the writer's own tests: some 300 blocks' worth of records in ragged input blocks"""
    d = tmp_path_factory.mktemp("block_writer_inputs")
    contigs, refs, recs = tl.fuzz_dataset(4402, 6000, with_rg=True)
    tl.write_bam(d / "fuzz.bam", refs, recs, level=1, rng=np.random.default_rng(5), block=6000)
    return d / "fuzz.bam"


def reblock(bins, src, dst, *more):
    return subprocess.run([str(bins / "hostcheck"), "-a", str(src), "-w", str(dst), "-b", *more], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("src", ["setA", "setB", "fuzz"])
def test_blocks_are_written_as_they_are(bins, fuzz_bam, tmp_path, src):
    path = fuzz_bam if src == "fuzz" else GOLD / f"{src}.bam"
    out = tmp_path / "out.bam"
    pr = reblock(bins, path, out)
    assert pr.returncode == 0, pr.stderr
    assert not Path(str(out) + ".tmp").exists()
    data = out.read_bytes()
    want = tl.bgzf_inflate(path.read_bytes())
    hb = header_bytes(want)
    assert data[-28:] == dl.EOF_BLOCK
    blocks = dl.walk(data)
    assert blocks[-1][1] == b"" and all(p for _, p in blocks[:-1])
    assert b"".join(p for _, p in blocks) == want
    # the header in blocks of its own, then the record stream cut every 0xFF00 bytes, whatever the records are
    n_head = -(-hb // dl.PAYLOAD)
    assert sum(len(p) for _, p in blocks[:n_head]) == hb
    body = blocks[n_head:-1]
    assert [len(p) for _, p in body] == [min(dl.PAYLOAD, len(want) - hb - k * dl.PAYLOAD) for k in range(len(body))]
    if src == "fuzz":
        assert len(body) > 16      # (more blocks than the five piece sizes: every one of them was used, several times)
    # the blocks are the ones zlib level 1 writes for these payloads: nothing was recompressed on the way
    for _, p in body[:3]:
        assert tl.bgzf_block(p, 1) in data
    sam = lambda p: subprocess.run([str(bins / "bam2sam"), str(p)], capture_output=True, text=True, check=True).stdout
    text = sam(path)
    assert sam(out) == text and text.count("\n") > 400


@pytest.mark.parametrize("damage,message", [("trunc", "ends inside a BGZF block"), ("chain", "BGZF")])
def test_a_piece_that_is_not_whole_blocks_fails_and_leaves_no_file(bins, tmp_path, damage, message):
    out = tmp_path / "out.bam"
    pr = reblock(bins, GOLD / "setA.bam", out, "-x", damage)
    assert pr.returncode == 1 and message in pr.stderr, pr.stderr
    assert not list(tmp_path.iterdir())

"""pss-bam -O ... -Z end to end on the GPU: the BAM whose blocks the device deflated holds the bytes the host writer's file
holds, every block of it passes deflate_lib.walk (Python's zlib), it ends in the EOF block, two runs write the same file, the
reports are those of the run without -O, and the file goes back in through the project's own device feed -- records
crossing blocks included -- to give the tables of the kept set.  The refusals end the command before any work."""
import gzip
from pathlib import Path

import numpy as np
import pytest

import deflate_lib as dl
import pssbam_testlib as tl
from test_gpu_cli_select import header_bytes, pkg, report_body, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
FA, BAM = GOLD / "setA.fa", GOLD / "setA.bam"
ARGS = ["-q", "20"]


@pytest.fixture(scope="module")
def fuzz_input(tmp_path_factory):
    """setA keeps less than one block's worth of records under any option; this input keeps several, so that records cross
    the blocks of the file written"""
    d = tmp_path_factory.mktemp("cli_deflate_inputs")
    contigs, refs, recs = tl.fuzz_dataset(4403, 4000, with_rg=True)
    tl.write_fasta(d / "fuzz.fa", contigs)
    tl.write_bam(d / "fuzz.bam", refs, recs, level=1)
    return d / "fuzz.fa", d / "fuzz.bam"


@pytest.mark.parametrize("src", ["setA", "fuzz"])
def test_cli_Z(pkg, tmp_path, fuzz_input, src):
    FA, BAM = (GOLD / "setA.fa", GOLD / "setA.bam") if src == "setA" else fuzz_input
    out, host = tmp_path / "kept.bam", tmp_path / "host.bam"
    pr = run_cli(pkg, FA, BAM, tmp_path / "out", *ARGS, "-O", str(out), "-Z")
    data = out.read_bytes() if out.exists() else b""
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(f" -O {out} -Z")
    assert not Path(str(out) + ".tmp").exists()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["kept.bam", "out.pss.counts.txt", "out.pss.rates.txt"]
    pz = run_cli(pkg, FA, BAM, tmp_path / "hostrun", *ARGS, "-O", str(host), "-z", "1")
    assert pz.returncode == 0, pz.stderr
    raw = gzip.decompress(host.read_bytes())
    assert gzip.decompress(data) == raw
    assert data[-28:] == dl.EOF_BLOCK
    blocks = dl.walk(data)
    assert b"".join(p for _, p in blocks) == raw and blocks[-1][1] == b"" and all(p for _, p in blocks[:-1])
    assert all(len(b) <= len(p) + dl.STORED_EXTRA for b, p in blocks) and len(data) < len(raw)
    # the device's blocks: the record stream behind the header, cut every 0xFF00 bytes
    hb = header_bytes(raw)
    n_rec = len(raw) - hb
    assert 0 < n_rec < len(gzip.decompress(BAM.read_bytes())) - hb
    if src == "fuzz":
        assert n_rec > 2 * dl.PAYLOAD      # (records cross blocks)
    assert [len(p) for _, p in blocks[:-1]] == [hb] + [min(dl.PAYLOAD, n_rec - k * dl.PAYLOAD) for k in range(-(-n_rec // dl.PAYLOAD))]
    # the same file again
    again = tmp_path / "again.bam"
    p2 = run_cli(pkg, FA, BAM, tmp_path / "out2", *ARGS, "-O", str(again), "-Z")
    assert p2.returncode == 0 and again.read_bytes() == data
    # reports and stdout: those of the run without -O
    plain = run_cli(pkg, FA, BAM, tmp_path / "plain", *ARGS)
    assert plain.returncode == 0 and plain.stdout == pr.stdout
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"out.pss.{kind}.txt").read_text()) == report_body((tmp_path / f"plain.pss.{kind}.txt").read_text()), kind
    # back in through the device feed (records cross these blocks): the tables of the kept set, every record kept
    back = run_cli(pkg, FA, out, tmp_path / "back", env={"PSSBAM_STATS": "1"})
    assert back.returncode == 0, back.stderr
    gf, gr = tl.parse_counts_text((tmp_path / "back.pss.counts.txt").read_text())
    wf, wr = tl.parse_counts_text((tmp_path / "out.pss.counts.txt").read_text())
    assert np.array_equal(gf, wf) and np.array_equal(gr, wr) and wf[2:].sum() > 0


@pytest.mark.parametrize("name", ["Z_alone", "Z_z", "Z_sam"])
def test_refusals(pkg, tmp_path, name):
    out = tmp_path / "o.bam"
    pr = {
        "Z_alone": lambda: run_cli(pkg, FA, BAM, tmp_path / "out", "-Z"),
        "Z_z": lambda: run_cli(pkg, FA, BAM, tmp_path / "out", "-O", str(out), "-Z", "-z", "1"),
        "Z_sam": lambda: run_cli(pkg, FA, GOLD / "setA.sam", tmp_path / "out", "-O", str(out), "-Z"),
    }[name]()
    assert pr.returncode != 0 and len(pr.stderr.splitlines()) == 1 and "Full command" not in pr.stderr, pr.stderr
    assert {"Z_alone": "needs -O", "Z_z": "-z", "Z_sam": "SAM text"}[name] in pr.stderr
    assert not list(tmp_path.iterdir())

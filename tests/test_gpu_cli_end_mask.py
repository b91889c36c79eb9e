"""pss-bam -O ... -K end to end on the GPU: the file holds the header and end_mask_lib.mask_record of the records the same
command writes without -K, with zlib on the host and with -Z; the reports are byte for byte those of the run without -K; the
files end in the EOF block."""
import gzip
from pathlib import Path

import pytest

import deflate_lib as dl
import end_mask_lib as em
from test_gpu_cli_select import pkg, run_cli  # noqa: F401

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
FA, BAM = GOLD / "setD.fa", GOLD / "setD.bam"


def test_cli_K(pkg, tmp_path):
    prefix = tmp_path / "p"                                   # the same prefix every time: the reports name it
    reports = lambda: {k: (tmp_path / f"p.pss.{k}.txt").read_bytes() for k in ("counts", "rates")}
    plain_bam = tmp_path / "plain.bam"
    p0 = run_cli(pkg, FA, BAM, prefix, "-q", "20", "-O", str(plain_bam))
    assert p0.returncode == 0, p0.stderr
    want_reports = reports()
    raw = gzip.decompress(plain_bam.read_bytes())
    hb = em.header_bytes(raw)
    want = raw[:hb] + em.mask_stream(raw[hb:], "ds", 3, 3)
    assert len(raw) > hb and want != raw and raw[:hb] == gzip.decompress(BAM.read_bytes())[:hb]
    for more in ([], ["-Z"]):
        out = tmp_path / ("k_Z.bam" if more else "k.bam")
        pr = run_cli(pkg, FA, BAM, prefix, "-q", "20", "-O", str(out), *more, "-K", "ds,3")
        assert pr.returncode == 0, pr.stderr
        assert pr.stderr.splitlines()[0].endswith(f" -O {out} {'-Z' if more else '-z 1'} -K ds,3,3")
        data = out.read_bytes()
        assert data[-28:] == dl.EOF_BLOCK and not Path(str(out) + ".tmp").exists()
        blocks = dl.walk(data)                                # every block: magic, BSIZE, CRC-32, ISIZE
        assert b"".join(p for _, p in blocks) == want == gzip.decompress(data)
        assert reports() == want_reports and pr.stdout == p0.stdout
    assert sorted(p.name for p in tmp_path.iterdir()) == ["k.bam", "k_Z.bam", "p.pss.counts.txt", "p.pss.rates.txt", "plain.bam"]


def test_K_without_O_is_refused_on_real_inputs(pkg, tmp_path):
    pr = run_cli(pkg, FA, BAM, tmp_path / "p", "-K", "ds,3")
    assert pr.returncode == 1 and len(pr.stderr.splitlines()) == 1 and "needs -O" in pr.stderr and not list(tmp_path.iterdir())

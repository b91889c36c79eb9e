"""pss-bam -c / -b end to end on the GPU: <prefix>.pss.coverage.txt and the bedGraph are what coverage_lib, the Python restatement,
gives for the records read back from the -O file of the same run -- per-base depth over kept.bam with no further filter, and its
`bedtools genomecov -bg` -- and, on SAM text, for the records the CPU oracle tallies."""
import os
import subprocess
from pathlib import Path

import pytest

import __graft_entry__ as ge
import coverage_lib as cl
import duplicates_lib as dl
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert (p.PKG_DIR / "bin" / "pss-bam").exists(), "front ends not built (run __graft_entry__.build())"
    return p


def run_cli(pkg, fa, aln, prefix, *more, env=None):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), *more], capture_output=True, text=True,
                          env={**os.environ, **(env or {})}, timeout=300)


def setd_with_copies(tmp_path):
    """setD.bam's records, every third of them once more right behind the file's end: duplicates for -d, depth for everyone"""
    refs, raw = tl.read_bam(GOLD / "setD.bam")
    blobs = dl.split_raw(raw)
    hdr = tl.bgzf_inflate((GOLD / "setD.bam").read_bytes())[:len(tl.bgzf_inflate((GOLD / "setD.bam").read_bytes())) - len(bytes(raw))]
    body = hdr + b"".join(blobs + blobs[::3])
    aln = tmp_path / "in.bam"
    aln.write_bytes(b"".join(tl.bgzf_block(body[i:i + 0xFF00]) for i in range(0, len(body), 0xFF00)) + tl.BGZF_EOF)
    return aln


@pytest.mark.parametrize("more", [[], ["-d", "-Z"]], ids=["plain", "d_Z"])
def test_c_and_b_equal_the_model_over_the_kept_bam(pkg, tmp_path, more):
    fa, aln = GOLD / "setD.fa", setd_with_copies(tmp_path)
    bg, kept = tmp_path / "x.bedgraph", tmp_path / "kept.bam"
    pr = run_cli(pkg, fa, aln, tmp_path / "out", "-q", "20", "-c", "-b", str(bg), "-O", str(kept), *more)
    assert pr.returncode == 0, pr.stderr
    assert f" -c -b {bg}" in pr.stderr.splitlines()[0]
    refs, raw = tl.read_bam(kept)
    contigs = {n: len(s) for n, s in dl.read_fasta(fa)}
    want = cl.from_raw(raw, refs, contigs)
    assert want.n_runs > 100 and int(want.hist[2:].sum()) > 0
    assert (tmp_path / "out.pss.coverage.txt").read_text() == cl.coverage_text(str(fa), str(aln), refs, contigs, want)
    assert bg.read_text() == cl.bedgraph_text(refs, want.runs)
    names = {p.name for p in tmp_path.iterdir()}
    assert names == {"in.bam", "kept.bam", "x.bedgraph", "out.pss.coverage.txt", "out.pss.counts.txt", "out.pss.rates.txt"} | ({"out.pss.duplicates.txt"} if more else set())
    if more:       # the deduplicated coverage is a smaller one
        plain = tmp_path / "plain"
        plain.mkdir()
        assert run_cli(pkg, fa, aln, plain / "out", "-q", "20", "-c").returncode == 0
        assert (plain / "out.pss.coverage.txt").read_text() != (tmp_path / "out.pss.coverage.txt").read_text()
        assert sorted(p.name for p in plain.iterdir()) == ["out.pss.counts.txt", "out.pss.coverage.txt", "out.pss.rates.txt"]


def test_b_alone_writes_no_summary(pkg, tmp_path):
    bg = tmp_path / "x.bedgraph"
    pr = run_cli(pkg, GOLD / "setD.fa", GOLD / "setD.bam", tmp_path / "out", "-b", str(bg))
    assert pr.returncode == 0, pr.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.counts.txt", "out.pss.rates.txt", "x.bedgraph"] and bg.stat().st_size > 0


def test_sam_text_without_O_against_the_oracles_verdicts(pkg, oracle, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(7301, 400)
    o = tl.PssOpts(region_len=10, min_mq=20)
    fa, sam, one = tmp_path / "g.fa", tmp_path / "in.sam", tmp_path / "one.sam"
    tl.write_fasta(fa, contigs)
    tl.write_sam(sam, refs, recs)
    g = oracle.load_genome(fa)
    try:
        idx = {n: i for i, (n, _) in enumerate(refs)}
        spans = []
        for r in recs:
            tl.write_sam(one, refs, [r])
            if oracle.pss(g, one, o)[2][tl.ST_OK]:
                spans.append(cl.span(cl.core_of_rec(r, idx)))
    finally:
        oracle.free_genome(g)
    one.unlink()
    assert 50 < len(spans) < len(recs)
    lens = {n: len(s) for n, s in contigs}
    want = cl.from_spans(spans, refs, lens)
    bg = tmp_path / "x.bedgraph"
    pr = run_cli(pkg, fa, sam, tmp_path / "out", *o.argv(), "-c", "-b", str(bg))
    assert pr.returncode == 0, pr.stderr
    assert (tmp_path / "out.pss.coverage.txt").read_text() == cl.coverage_text(str(fa), str(sam), refs, lens, want)
    assert bg.read_text() == cl.bedgraph_text(refs, want.runs)


def test_a_failed_run_leaves_no_tmp_file_and_no_bedgraph(pkg, tmp_path):
    # fails before the tally: a FASTA that is not there
    bg = tmp_path / "x.bedgraph"
    pr = run_cli(pkg, tmp_path / "none.fa", GOLD / "setD.bam", tmp_path / "out", "-c", "-b", str(bg))
    assert pr.returncode == 1 and "Unable to load genome" in pr.stderr, pr.stderr
    assert not list(tmp_path.iterdir())
    # fails at the last step, the rename: -b names an existing directory
    bg.mkdir()
    pr = run_cli(pkg, GOLD / "setD.fa", GOLD / "setD.bam", tmp_path / "out", "-b", str(bg), env={"PSSBAM_DETACH_EXIT": "0"})
    assert pr.returncode == 1, pr.stderr
    assert "Cannot write to file" in pr.stderr and bg.is_dir() and not list(bg.iterdir())
    assert not any(p.name.endswith(".tmp") for p in tmp_path.iterdir())

"""pss-bam -w end to end on the GPU: <prefix>.pss.windows.txt and <prefix>.pss.gcbias.txt are what windows_lib, the Python
restatement, gives for the records read back from the -O file of the same run and the FASTA's letters -- and, on SAM text, for the
records the CPU oracle tallies.  The helpers are those of test_gpu_cli_coverage."""
import pytest

import __graft_entry__ as ge
import coverage_lib as cl
import duplicates_lib as dl
import pssbam_testlib as tl
import test_gpu_cli_coverage as tcc
import windows_lib as wl

pytestmark = pytest.mark.gpu

GOLD = tcc.GOLD


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert (p.PKG_DIR / "bin" / "pss-bam").exists(), "front ends not built (run __graft_entry__.build())"
    return p


def test_w_alone_writes_the_two_files_and_no_coverage_report(pkg, tmp_path):
    pr = tcc.run_cli(pkg, GOLD / "setD.fa", GOLD / "setD.bam", tmp_path / "out", "-w", "64")
    assert pr.returncode == 0, pr.stderr
    assert " -w 64" in pr.stderr.splitlines()[0]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.counts.txt", "out.pss.gcbias.txt", "out.pss.rates.txt", "out.pss.windows.txt"]
    lines = (tmp_path / "out.pss.windows.txt").read_text().splitlines()
    assert lines[3:6] == ["# window: 64", "# windows: 95", "contig\tstart\tend\tacgt\tgc\tgc_fraction\tcovered\tdepth_sum\tmean_depth"] and len(lines) == 6 + 95
    assert sum(int(ln.split("\t")[7]) for ln in lines[6:]) > 0
    assert len((tmp_path / "out.pss.gcbias.txt").read_text().splitlines()) == 8 + 101


def test_w_with_c_b_O_d_Z_equals_the_model_over_the_kept_bam(pkg, tmp_path):
    fa, aln = GOLD / "setD.fa", tcc.setd_with_copies(tmp_path)
    bg, kept = tmp_path / "x.bedgraph", tmp_path / "kept.bam"
    pr = tcc.run_cli(pkg, fa, aln, tmp_path / "out", "-q", "20", "-w", "64", "-c", "-b", str(bg), "-O", str(kept), "-d", "-Z")
    assert pr.returncode == 0, pr.stderr
    refs, raw = tl.read_bam(kept)
    seqs = dict(dl.read_fasta(fa))
    lens = {n: len(s) for n, s in seqs.items()}
    win = wl.from_raw(raw, refs, seqs, 64)
    assert int(win[6].sum()) > 0 and (win[2] - win[1] < 64).any()
    assert (tmp_path / "out.pss.windows.txt").read_text() == wl.windows_text(str(fa), str(aln), refs, 64, win)
    assert (tmp_path / "out.pss.gcbias.txt").read_text() == wl.gcbias_text(str(fa), str(aln), 64, win)
    # the other reports of the same run are what they are without -w, and a contig's windows sum to its line of -c
    want = cl.from_raw(raw, refs, lens)
    cov = (tmp_path / "out.pss.coverage.txt").read_text()
    assert cov == cl.coverage_text(str(fa), str(aln), refs, lens, want) and bg.read_text() == cl.bedgraph_text(refs, want.runs)
    by_name = {ln.split("\t")[0]: ln.split("\t") for ln in cov.splitlines()[4:4 + len(refs)]}
    rows = [ln.split("\t") for ln in (tmp_path / "out.pss.windows.txt").read_text().splitlines()[6:]]
    for n, _ in refs:
        mine = [r for r in rows if r[0] == n]
        assert sum(int(r[6]) for r in mine) == int(by_name[n][2]) and sum(int(r[7]) for r in mine) == int(by_name[n][4])
    assert {p.name for p in tmp_path.iterdir()} == {"in.bam", "kept.bam", "x.bedgraph", "out.pss.coverage.txt", "out.pss.counts.txt", "out.pss.rates.txt",
                                                    "out.pss.duplicates.txt", "out.pss.windows.txt", "out.pss.gcbias.txt"}


def test_sam_text_against_the_oracles_verdicts(pkg, oracle, tmp_path):
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
    win = wl.from_spans(spans, refs, dict(contigs), 100)
    assert (win[3] < win[2] - win[1]).any()                                                # (letters that are no A C G T)
    pr = tcc.run_cli(pkg, fa, sam, tmp_path / "out", *o.argv(), "-w", "100")
    assert pr.returncode == 0, pr.stderr
    assert (tmp_path / "out.pss.windows.txt").read_text() == wl.windows_text(str(fa), str(sam), refs, 100, win)
    assert (tmp_path / "out.pss.gcbias.txt").read_text() == wl.gcbias_text(str(fa), str(sam), 100, win)
    assert not (tmp_path / "out.pss.coverage.txt").exists()


def test_two_failing_runs_leave_no_file(pkg, tmp_path):
    # fails before the tally: a FASTA that is not there
    pr = tcc.run_cli(pkg, tmp_path / "none.fa", GOLD / "setD.bam", tmp_path / "out", "-w", "64")
    assert pr.returncode == 1 and "Unable to load genome" in pr.stderr, pr.stderr
    assert not list(tmp_path.iterdir())
    # fails at the last step, the second rename: the GC-bias file's name is taken by a directory
    taken = tmp_path / "out.pss.gcbias.txt"
    taken.mkdir()
    pr = tcc.run_cli(pkg, GOLD / "setD.fa", GOLD / "setD.bam", tmp_path / "out", "-w", "64", env={"PSSBAM_DETACH_EXIT": "0"})
    assert pr.returncode == 1, pr.stderr
    assert "Cannot write to file" in pr.stderr and taken.is_dir() and not list(taken.iterdir())
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.counts.txt", "out.pss.gcbias.txt", "out.pss.rates.txt"]

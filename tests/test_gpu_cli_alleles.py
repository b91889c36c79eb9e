"""pss-bam -a / -t end to end on the GPU: <prefix>.pss.alleles.txt is what alleles_lib, the Python restatement, gives for the records
read back from the -O file of the same run -- a strand-split pileup over kept.bam with no further filter -- the other files of the
run are those of the run without -a, SAM text gives the same counts, and what is refused leaves nothing behind."""
import os
import subprocess
from pathlib import Path

import pytest

import __graft_entry__ as ge
import alleles_lib as al
import duplicates_lib as dl
import pssbam_testlib as tl
from test_gpu_cli_coverage import setd_with_copies

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert (p.PKG_DIR / "bin" / "pss-bam").exists(), "front ends not built (run __graft_entry__.build())"
    return p


def run_cli(pkg, fa, aln, prefix, *more, env=None, tool="pss-bam"):
    exe = pkg.PKG_DIR / "bin" / tool
    return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), *more], capture_output=True, text=True,
                          env={**os.environ, **(env or {})}, timeout=300)


def sites_file(tmp_path, seqs) -> tuple:
    """every third position of setD's contigs in a shuffled order with a duplicate, a contig the genome lacks, a position beyond a
    contig's end, extra columns and a comment"""
    import numpy as np
    sites = [(n, p) for n, q in seqs.items() for p in range(1, len(q), 3)]
    order = np.random.default_rng(79).permutation(len(sites))
    name = next(iter(seqs))
    sites = [sites[j] for j in order] + [sites[0], ("no_such_contig", 4), (name, len(seqs[name]))]
    path = tmp_path / "panel.sites"
    path.write_text("# a panel\n" + "".join(f"{n}\t{p + 1}\trs{k}\tA\tG\n" if k % 2 else f"{n} {p + 1}\n" for k, (n, p) in enumerate(sites)))
    return path, sites


@pytest.mark.parametrize("more,trim,min_bq", [([], 0, 0), (["-d", "-q", "20", "-Q", "20", "-t", "2"], 2, 20)], ids=["plain", "d_q_Q_t"])
def test_a_equals_the_model_over_the_kept_bam_and_changes_no_other_file(pkg, tmp_path, more, trim, min_bq):
    fa, aln = GOLD / "setD.fa", setd_with_copies(tmp_path)
    seqs = dict(dl.read_fasta(fa))
    panel, sites = sites_file(tmp_path, seqs)
    kept = tmp_path / "kept.bam"
    pr = run_cli(pkg, fa, aln, tmp_path / "out", "-a", str(panel), "-O", str(kept), *more)
    assert pr.returncode == 0, pr.stderr
    assert f" -a {panel} -t {trim}" in pr.stderr.splitlines()[0]
    refs, raw = tl.read_bam(kept)
    want = al.report_of_raw(fa, aln, panel, trim, refs, seqs, raw, sites, min_bq)
    got = (tmp_path / "out.pss.alleles.txt").read_text()
    assert got == want
    head = got.splitlines()[1].split()
    assert int(head[2]) == len(set(sites)) and int(head[4]) == len(set(sites)) - 2 and int(head[6]) > 50 and int(head[8]) > 500
    names = {p.name for p in tmp_path.iterdir()}
    assert names == {"in.bam", "kept.bam", "panel.sites", "out.pss.alleles.txt", "out.pss.counts.txt", "out.pss.rates.txt"} | ({"out.pss.duplicates.txt"} if more else set())
    plain = tmp_path / "plain"
    plain.mkdir()
    assert run_cli(pkg, fa, aln, plain / "out", "-O", str(plain / "kept.bam"), *[m for m in more if m not in ("-t", "2")]).returncode == 0
    norm = lambda b: b.replace(str(plain).encode(), b"").replace(str(tmp_path).encode(), b"")  # noqa: E731
    for f in ("out.pss.counts.txt", "out.pss.rates.txt"):
        assert norm((plain / f).read_bytes()) == norm((tmp_path / f).read_bytes()), f
    assert (plain / "kept.bam").read_bytes() == kept.read_bytes()
    assert not (plain / "out.pss.alleles.txt").exists()


def test_sam_text_gives_the_counts_of_the_bam(pkg, tmp_path):
    fa = GOLD / "setD.fa"
    seqs = dict(dl.read_fasta(fa))
    panel, sites = sites_file(tmp_path, seqs)
    kept = tmp_path / "kept.bam"
    assert run_cli(pkg, fa, GOLD / "setD.bam", tmp_path / "bam", "-a", str(panel), "-t", "1", "-O", str(kept)).returncode == 0
    pr = run_cli(pkg, fa, GOLD / "setD.sam", tmp_path / "sam", "-a", str(panel), "-t", "1")
    assert pr.returncode == 0, pr.stderr
    a, b = (tmp_path / "bam.pss.alleles.txt").read_text().splitlines(), (tmp_path / "sam.pss.alleles.txt").read_text().splitlines()
    assert a[0].replace("setD.bam", "setD.sam") == b[0] and a[1:] == b[1:] and len(a) > 100
    refs, raw = tl.read_bam(kept)
    assert "\n".join(b) + "\n" == al.report_of_raw(fa, GOLD / "setD.sam", panel, 1, refs, seqs, raw, sites)


def test_what_is_refused_leaves_nothing_behind(pkg, tmp_path):
    fa, bam = GOLD / "setD.fa", GOLD / "setD.bam"
    work = tmp_path / "w"
    work.mkdir()
    panel, _ = sites_file(tmp_path, dict(dl.read_fasta(fa)))
    bad = tmp_path / "bad.sites"
    bad.write_text("ctg1\t5\nctg1\tfive\n")

    def refused(pr, *parts):
        assert pr.returncode == 1 and all(p in pr.stderr for p in parts), pr.stderr
        assert not list(work.iterdir())

    refused(run_cli(pkg, fa, bam, work / "out", "-a", str(panel), "-I"), "-a", "-I", "does not go with")
    refused(run_cli(pkg, fa, bam, work / "out", "-t", "2"), "-t", "needs -a")
    refused(run_cli(pkg, fa, bam, work / "out", "-a", str(panel), "-t", "65536"), "-t takes a number of bases in 0..65535")
    refused(run_cli(pkg, fa, bam, work / "out", "-a", str(bad)), f"-a: {bad}: line 2:", "not a decimal integer")
    refused(run_cli(pkg, fa, bam, work / "out", "-a", str(panel), env={"PSSBAM_NGPU": "2"}), "-a", "PSSBAM_NGPU=2")
    refused(run_cli(pkg, fa, bam, work / "out", "-k", "4", "-a", str(panel), tool="fragkon"), "-a", "is an option of pss-bam")
    refused(run_cli(pkg, fa, bam, work / "out", "-k", "4", "-t", "2", tool="fragkon"), "-t", "is an option of pss-bam")
    # a run that fails after the options were taken: a FASTA that is not there
    pr = run_cli(pkg, tmp_path / "none.fa", bam, work / "out", "-a", str(panel))
    assert pr.returncode == 1 and "Unable to load genome" in pr.stderr and not list(work.iterdir())

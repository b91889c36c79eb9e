"""Drop-in boundary, from the reference's side: the UNMODIFIED reference `main`s
(pss-bam.c:650-805, fragkon.c:253-386, genome-kmer-count.c:23-66) compiled against THIS repo's
include/{fasta-genome-io,sam-parse,kmer}.h and linked with libpssbam_host.so instead of the
reference's own fasta-genome-io.c / sam-parse.c / kmer.c, then run on the golden inputs: their
output must be the golden files byte for byte.

The binaries are oracle/_ref/on_ours/*, made by build() through oracle/Makefile where the
reference sources are present; the reference source never enters the repository, and this
module reads nothing outside it.  Skipped where build() had no reference sources to compile."""
import json
import subprocess
from pathlib import Path

import pytest

import pssbam_testlib as tl

GOLD = Path(__file__).resolve().parent / "golden"
MANIFEST = json.loads((GOLD / "manifest.json").read_text())
MAINS = tl.REF_DIR / "on_ours"
TOOLS = ("pss-bam", "fragkon", "genome-kmer-count")

pytestmark = pytest.mark.skipif(not all((MAINS / t).exists() for t in TOOLS),
                                reason="oracle/_ref/on_ours not built (no reference sources at build time)")


@pytest.fixture(scope="module")
def ref_mains():
    return {t: MAINS / t for t in TOOLS}


def _stage(ds, tmp_path):
    for k in ("fasta", "sam"):
        (tmp_path / ds[k]).write_bytes((GOLD / ds[k]).read_bytes())


@pytest.mark.parametrize("case", [c for c in MANIFEST["cases"] if c["tool"] == "pss-bam"], ids=lambda c: c["prefix"])
def test_reference_pss_main_on_our_headers_and_library(ref_mains, case, tmp_path):
    ds = MANIFEST["datasets"][case["dataset"]]
    _stage(ds, tmp_path)
    o = tl.PssOpts(**case["opts"])
    pr = subprocess.run([str(ref_mains["pss-bam"]), "-F", ds["fasta"], "-B", ds["sam"], "-o", case["prefix"]] + o.argv(),
                        cwd=tmp_path, env=tl._ref_env(), capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert (tmp_path / case["counts"]).read_text() == (GOLD / case["counts"]).read_text()
    assert (tmp_path / case["rates"]).read_text() == (GOLD / case["rates"]).read_text()


@pytest.mark.parametrize("case", [c for c in MANIFEST["cases"] if c["tool"] == "fragkon"], ids=lambda c: c["stdout"])
def test_reference_fragkon_main_on_our_headers_and_library(ref_mains, case, tmp_path):
    ds = MANIFEST["datasets"][case["dataset"]]
    _stage(ds, tmp_path)
    o = tl.FkOpts(**case["opts"])
    # fragkon.c:372 frees an uninitialised pointer after printing: line-buffer stdout, accept that abort
    pr = subprocess.run(["stdbuf", "-oL", str(ref_mains["fragkon"]), "-F", ds["fasta"], "-B", ds["sam"]] + o.argv(),
                        cwd=tmp_path, env=tl._ref_env(), capture_output=True, text=True, timeout=300)
    assert pr.returncode in (0, -6, -11), pr.stderr[-2000:]
    assert pr.stdout == (GOLD / case["stdout"]).read_text()


@pytest.mark.parametrize("case", [c for c in MANIFEST["cases"] if c["tool"] == "genome-kmer-count"],
                         ids=lambda c: c["stdout"])
def test_reference_gkc_main_on_our_headers_and_library(ref_mains, case, tmp_path):
    ds = MANIFEST["datasets"][case["dataset"]]
    (tmp_path / ds["fasta"]).write_bytes((GOLD / ds["fasta"]).read_bytes())
    pr = subprocess.run([str(ref_mains["genome-kmer-count"]), "-f", ds["fasta"], "-k", str(case["klen"])],
                        cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    assert pr.stdout == (GOLD / case["stdout"]).read_text()

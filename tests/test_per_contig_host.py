"""pss-bam -A without a GPU: the C ABI carries the setter and the reader of the planes, the command line knows the
option and refuses it together with the other splits before any work, and the writer of <prefix>.pss.contigs.txt
writes, for hand-made tables, exactly the rows of each contig's counts file behind the contig's name."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_pkg()


def test_symbols_are_declared_listed_and_exported(pkg):
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^int pssbam_engine_set_per_contig\(pssbam_engine \*e, int32_t on\);$", hdr, re.M)
    assert re.search(r"^int pssbam_engine_finish_contigs\(pssbam_engine \*e, int32_t first_ref, int32_t n, unsigned long \*fwd, "
                     r"unsigned long \*rev,\n\s+uint8_t \*touched\);$", hdr, re.M)
    L = pkg.hip_lib()
    L.pssbam_last_error.restype = C.c_char_p
    for s in ("pssbam_engine_set_per_contig", "pssbam_engine_finish_contigs"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert L.pssbam_engine_set_per_contig(None, 1) == -1                       # PSSBAM_EINVAL, not a dereference
    assert L.pssbam_engine_finish_contigs(None, 0, 1, None, None, None) == -1
    assert L.pssbam_last_error()
    for name in ("set_per_contig", "finish_contigs", "per_contig"):
        assert hasattr(pkg.Engine, name)
    H = C.CDLL(str(pkg.PKG_DIR / "libpssbam_host.so"))
    assert hasattr(H, "pss_write_contigs")


REFUSED = [(["-A", "-G"], "-G"), (["-G", "-A"], "-G"), (["-A", "-S", "40"], "-S"), (["-A", "-C", "no.map"], "-C"),
           (["-H", "100", "-A"], "-H"), (["-X", "cpg", "-A"], "-X"), (["-A", "-E", "ss"], "-E"), (["-I", "-A"], "-I")]


@pytest.mark.parametrize("args,word", REFUSED)
def test_cli_refuses_the_other_splits_before_any_work(pkg, args, word, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(tmp_path / "no.fa"), "-B", str(tmp_path / "no.bam"), "-o", str(tmp_path / "out"), *args],
                        capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    lines = pr.stderr.splitlines()
    assert len(lines) == 1 and lines[0].startswith("-A (tables per contig) and ") and word in lines[0], pr.stderr
    assert lines[0].endswith(" exclude each other.")
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr
    assert pr.stdout == "" and list(tmp_path.iterdir()) == []


def test_cli_usage_names_the_option_and_fragkon_has_none(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-A"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr
    assert len([ln for ln in pr.stderr.splitlines() if ln.startswith("-A <")]) == 1
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "fragkon"), "-A"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -A." in pr.stderr


def test_cli_goes_with_R_Q_T(pkg, tmp_path):
    """with -R, -Q and -T the option passes the check of the exclusive options: the command gets as far as the BED file it
    cannot read, the next thing it looks at, and ends there before any work (the banner with -A and the files are the GPU
    tests' business)"""
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-F", str(tmp_path / "no.fa"), "-B", str(tmp_path / "no.bam"), "-o",
                         str(tmp_path / "out"), "-A", "-R", "grpA", "-Q", "20", "-T", str(tmp_path / "no.bed")],
                        capture_output=True, text=True, timeout=60)
    lines = pr.stderr.splitlines()
    assert pr.returncode == 1 and len(lines) == 1 and "no.bed" in lines[0] and "exclude each other" not in pr.stderr, pr.stderr
    assert pr.stdout == "" and list(tmp_path.iterdir()) == []


def row(label: int, counts) -> str:
    return f"{label}\t" + "".join(f"{int(c)}\t" for c in counts) + "\n"


def test_contigs_writer_writes_exactly_the_specified_lines(pkg, tmp_path):
    H = C.CDLL(str(pkg.PKG_DIR / "libpssbam_host.so"))
    H.pss_write_contigs.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p]
    n_len, names = 3, [b"chrB", b"tiny.4 x", b"*"]
    rng = np.random.default_rng(11)
    fwd = rng.integers(0, 2 ** 40, size=(3, n_len + 2, 16)).astype(np.uint64)
    rev = rng.integers(0, 1000, size=(3, n_len + 2, 16)).astype(np.uint64)
    prefix = tmp_path / "rep"
    arr = (C.c_char_p * 3)(*names)
    assert H.pss_write_contigs(b"g.fa", b"in.bam", str(prefix).encode(), n_len, 3, arr, fwd.ctypes.data, rev.ctypes.data) == 0
    assert [p.name for p in tmp_path.iterdir()] == ["rep.pss.contigs.txt"]
    want = (f"### pss-bam.c v1.2.1:\n### FASTA: g.fa\n### BAM: in.bam\n### OUT: {prefix}.pss.contigs.txt\n"
            "### CONTIG TABLE POS AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT\n")
    for k, nm in enumerate(n.decode() for n in names):
        for r in range(n_len + 2):                                   # forward: -2 .. N-1
            want += f"{nm}\tfwd\t" + row(r - 2, fwd[k, r])
        for pos in range(n_len - 1, -1, -1):                         # reverse: N-1 .. 0, then 1, 2
            want += f"{nm}\trev\t" + row(pos, rev[k, pos + 2])
        want += f"{nm}\trev\t" + row(1, rev[k, 1]) + f"{nm}\trev\t" + row(2, rev[k, 0])
    assert (tmp_path / "rep.pss.contigs.txt").read_text() == want
    # the rows are those of a counts file of the same tables
    H.pss_write_counts.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
    assert H.pss_write_counts(b"g.fa", b"in.bam", str(tmp_path / "one").encode(), n_len, fwd[1].ctypes.data, rev[1].ctypes.data) == 0
    body = [ln for ln in (tmp_path / "one.pss.counts.txt").read_text().splitlines() if ln and not ln.startswith("#")]
    mine = [ln.split("\t", 2)[2] for ln in want.splitlines() if ln.startswith("tiny.4 x\t")]
    assert mine == body
    # no contig at all: the five header lines; an unwritable prefix: 1 after a diagnostic
    assert H.pss_write_contigs(b"g.fa", b"in.bam", str(tmp_path / "none").encode(), n_len, 0, arr, None, None) == 0
    assert len((tmp_path / "none.pss.contigs.txt").read_text().splitlines()) == 5
    assert H.pss_write_contigs(b"g.fa", b"in.bam", str(tmp_path / "no_such_dir" / "x").encode(), n_len, 0, arr, None, None) == 1

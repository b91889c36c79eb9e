"""fragkon -S / -G / -C without a GPU: the command line's option parsing and usage errors, the plane report writer of
libpssbam_host.so against a hand-made table, the new C-ABI symbol of libpssbam_hip.so, and the usage text."""
import ctypes as C
import re
import subprocess

import pytest

import __graft_entry__ as ge

# the usage text of the reference's fragkon, line for line
USAGE = ["fragkon: Program for describing kmer-based genomic sequence",
         "contexts around the fragmentation points of aligned reads.",
         "-F <reference FASTA (required)>",
         "-B <input BAM (required)>",
         "-k <kmer length (default: 8)>",
         "-l <minimum length of read to report (default: 0)>",
         "-L <maximum length of read to report (default: 250000000)>",
         "-q <map quality filter of read to report (default: 0)>",
         "-m <only consider merged reads>"]


def _run_cli(tmp_path, *args):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "fragkon"
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), *args],
                          capture_output=True, text=True, timeout=60)


def _one_line(pr):
    assert pr.returncode == 1
    assert "Unknown option" not in pr.stderr
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "Entered command" not in lines[0], pr.stderr
    return lines[0]


@pytest.mark.parametrize("args", [
    ["-S", ""], ["-S", "abc"], ["-S", "30,30"], ["-S", "40,30"], ["-S", "0"], ["-S", "30, 40"],
    ["-l", "30", "-S", "30"], ["-L", "80", "-S", "30,81"], ["-S", ",".join(str(v) for v in range(31, 95))],
])
def test_cli_refuses_bad_S_before_any_gpu_work(tmp_path, args):
    line = _one_line(_run_cli(tmp_path, "-o", str(tmp_path / "o"), *args))
    assert "-S" in line
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("args,flag", [(["-S", "40"], "-S"), (["-G"], "-G"), (["-C", "map.tsv"], "-C")])
def test_cli_selector_needs_o(tmp_path, args, flag):
    line = _one_line(_run_cli(tmp_path, *args))
    assert flag in line and "-o" in line
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("args", [["-S", "40", "-G"], ["-G", "-C", "map.tsv"], ["-C", "map.tsv", "-S", "40"], ["-S", "40", "-G", "-C", "m"]])
def test_cli_refuses_two_selectors(tmp_path, args):
    line = _one_line(_run_cli(tmp_path, "-o", str(tmp_path / "o"), *args))
    assert "-S" in line and "-G" in line and "-C" in line and "exclude" in line
    assert not list(tmp_path.iterdir())


def test_cli_refuses_bad_map_file(tmp_path):
    line = _one_line(_run_cli(tmp_path, "-o", str(tmp_path / "o"), "-C", str(tmp_path / "missing.tsv")))
    assert "-C" in line and "missing.tsv" in line
    (tmp_path / "twice.tsv").write_text("chr1\ta\nchr1\tb\n")
    line = _one_line(_run_cli(tmp_path, "-o", str(tmp_path / "o"), "-C", str(tmp_path / "twice.tsv")))
    assert "chr1" in line and "twice.tsv" in line


def test_usage_text_keeps_every_line(tmp_path):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "fragkon"
    for args in ([], ["-S", "40"], ["-G"], ["-C", "x"], ["-o", "p"]):      # the new options are known; no -F / -B: usage
        pr = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=60)
        assert pr.returncode == 1 and pr.stdout == ""
        assert "Unknown option" not in pr.stderr
        assert pr.stderr.splitlines()[:len(USAGE)] == USAGE


def test_plane_report_writer(tmp_path):
    """<prefix>.<tag>.fragkon.txt in fragkon_write_table's format: header echoing the -F / -B strings, one row per
    k-mer in ACGT order, counts sticking at UINT_MAX"""
    pkg = ge.load_pkg()
    host = C.CDLL(str(pkg.LIB_HOST))
    host.fragkon_write_plane.restype = C.c_int
    host.fragkon_write_plane.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]
    k5 = (C.c_uint64 * 16)(*range(16))
    k3 = (C.c_uint64 * 16)(*[100 + v for v in range(16)])
    k5[5], k5[6], k3[15] = 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7
    prefix = tmp_path / "out.dir" / "p"
    prefix.parent.mkdir()
    assert host.fragkon_write_plane(b"some genome.fa", b"../in.bam", str(prefix).encode(), b"len30-59", 2, k5, k3) == 0
    assert [p.name for p in prefix.parent.iterdir()] == ["p.len30-59.fragkon.txt"]
    lines = (prefix.parent / "p.len30-59.fragkon.txt").read_text().split("\n")
    assert lines[:4] == ["### fragkon.c v0.3", "### some genome.fa", "### ../in.bam", "# KMER\t5' CONTEXT COUNTS\t3' CONTEXT COUNTS"]
    assert lines[-1] == "" and len(lines) == 4 + 16 + 1
    kmers = [a + b for a in "ACGT" for b in "ACGT"]
    want5 = [min(int(v), 2 ** 32 - 1) for v in k5]
    want3 = [min(int(v), 2 ** 32 - 1) for v in k3]
    assert lines[4:20] == [f"{km}\t{a}\t{b}" for km, a, b in zip(kmers, want5, want3)]
    assert lines[4 + 6] == f"CG\t{2 ** 32 - 1}\t106" and lines[19] == f"TT\t15\t{2 ** 32 - 1}"
    # an unwritable place is a diagnosed failure
    assert host.fragkon_write_plane(b"g.fa", b"in.bam", str(tmp_path / "nowhere" / "p").encode(), b"x", 2, k5, k3) == 1


def test_kmer_plane_symbol_is_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    assert "pssbam_engine_finish_kmer_groups" in pkg.HIP_SYMBOLS and hasattr(L, "pssbam_engine_finish_kmer_groups")
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"int pssbam_engine_finish_kmer_groups\(pssbam_engine \*e, int32_t group, uint64_t \*k5, uint64_t \*k3\);", hdr)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)                  # additive: the ABI version stays
    assert L.pssbam_engine_finish_kmer_groups(None, 0, None, None) == -1       # a NULL engine is refused, not touched

"""pss-bam -H without a GPU: the limit parser and the lengths-file writer of libpssbam_host.so, the C-ABI symbols
of libpssbam_hip.so, and the command line's -H diagnostics."""
import ctypes as C
import re
import subprocess

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_length_hist.restype = C.c_int
    L.pss_parse_length_hist.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.pss_write_lengths.restype = C.c_int
    L.pss_write_lengths.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


def parse(host, arg: bytes):
    """the limit, or the diagnostic (str) of a rejection"""
    err = C.create_string_buffer(200)
    v = host.pss_parse_length_hist(arg, err, len(err))
    if v < 0:
        assert v == -1 and err.value and b"\n" not in err.value, arg
        return err.value.decode()
    return v


@pytest.mark.parametrize("arg,want", [(b"1", 1), (b"65535", 65535), (b"300", 300), (b"0300", 300)])
def test_parser_accepts(host, arg, want):
    assert parse(host, arg) == want


@pytest.mark.parametrize("arg", [b"0", b"65536", b"-1", b"12x", b"", b"+5", b" 5", b"5 ", b"3.5", b"0x10", b"99999999999999999999"])
def test_parser_rejects_with_a_message(host, arg):
    msg = parse(host, arg)
    assert isinstance(msg, str) and "-H" in msg


def test_parser_diagnostics_name_the_problem(host):
    assert "65535" in parse(host, b"65536")
    assert "decimal" in parse(host, b"12x")
    assert "at least 1" in parse(host, b"0")


def test_write_lengths_exact_bytes(host, tmp_path):
    m = 5
    fwd = (C.c_uint64 * (m + 2))(0, 7, 0, 2 ** 40 + 3, 0, 1, 9)
    rev = (C.c_uint64 * (m + 2))(0, 0, 0, 4, 5, 0, 2 ** 63)
    prefix = tmp_path / "out"
    assert host.pss_write_lengths(b"the genome.fa", b"in.bam", str(prefix).encode(), m, fwd, rev) == 0
    want = ("# fragment lengths of the reads added to the forward / reverse table\n"
            "# FASTA: the genome.fa\n"
            "# BAM: in.bam\n"
            "length\tfwd\trev\n"
            "0\t0\t0\n"
            "1\t7\t0\n"
            "2\t0\t0\n"
            f"3\t{2 ** 40 + 3}\t4\n"
            "4\t0\t5\n"
            "5\t1\t0\n"
            f">5\t9\t{2 ** 63}\n")
    assert (tmp_path / "out.pss.lengths.txt").read_bytes() == want.encode()
    assert [p.name for p in tmp_path.iterdir()] == ["out.pss.lengths.txt"]


def test_write_lengths_smallest_limit_and_unwritable_prefix(host, tmp_path):
    fwd, rev = (C.c_uint64 * 3)(1, 2, 3), (C.c_uint64 * 3)(4, 5, 6)
    assert host.pss_write_lengths(b"f", b"b", str(tmp_path / "o").encode(), 1, fwd, rev) == 0
    assert (tmp_path / "o.pss.lengths.txt").read_text().splitlines()[3:] == ["length\tfwd\trev", "0\t1\t4", "1\t2\t5", ">1\t3\t6"]
    assert host.pss_write_lengths(b"f", b"b", str(tmp_path / "no_such_dir" / "o").encode(), 1, fwd, rev) == 1


def test_length_hist_symbols_are_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_length_histogram", "pssbam_engine_finish_length_histogram"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert pkg.MAX_HIST_LENGTH == 65535
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_MAX_HIST_LENGTH 65535\b", hdr)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert re.search(r"int pssbam_engine_set_length_histogram\(pssbam_engine \*e, int32_t max_len\);", hdr)
    assert re.search(r"int pssbam_engine_finish_length_histogram\(pssbam_engine \*e, uint64_t \*fwd, uint64_t \*rev\);", hdr)
    assert L.pssbam_engine_set_length_histogram(None, 300) == -1      # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_length_histogram(None, None, None) == -1
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_length_hist", "pss_write_lengths"):
        assert hasattr(host, s)


def _run_cli(tmp_path, *args):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"),
                           *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [["-H", ""], ["-H", "0"], ["-H", "65536"], ["-H", "-1"], ["-H", "12x"]])
def test_cli_refuses_bad_H_before_any_gpu_work(tmp_path, args):
    pr = _run_cli(tmp_path, *args)
    assert pr.returncode == 1
    assert "Unknown option -H" not in pr.stderr
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-H" in lines[0] and "Full command" not in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())


@pytest.mark.parametrize("args,other", [(["-H", "120", "-G"], "-G"), (["-G", "-H", "120"], "-G"), (["-H", "120", "-S", "40"], "-S"),
                                        (["-H", "120", "-C", "no_such_map.tsv"], "-C")])
def test_cli_refuses_H_with_planes_before_any_gpu_work(tmp_path, args, other):
    pr = _run_cli(tmp_path, *args)
    assert pr.returncode == 1
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-H" in lines[0] and other in lines[0] and "exclude each other" in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())


def test_cli_knows_H(tmp_path):
    """-H takes an argument (the usage text is the reference's and stays as it is)"""
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-H", "40"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1
    assert "Unknown option" not in pr.stderr and pr.stderr.startswith("pss-bam v1.2.1:")

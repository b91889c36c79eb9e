"""pss-bam -S without a GPU: the length bin edge parser and the bin -> file-name tag of libpssbam_host.so,
the C-ABI symbol of libpssbam_hip.so, and the command line's -S diagnostics."""
import ctypes as C
import re
import subprocess

import pytest

import __graft_entry__ as ge

DEFAULT_L = 250000000


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_length_edges.restype = C.c_int
    L.pss_parse_length_edges.argtypes = [C.c_char_p, C.c_ulong, C.c_ulong, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
    L.pss_length_bin_tag.restype = C.c_size_t
    L.pss_length_bin_tag.argtypes = [C.c_ulong, C.c_ulong, C.c_char_p, C.c_size_t]
    L.pss_length_bin_bounds.restype = None
    L.pss_length_bin_bounds.argtypes = [C.POINTER(C.c_uint32), C.c_int, C.c_int, C.c_ulong, C.c_ulong,
                                        C.POINTER(C.c_ulong), C.POINTER(C.c_ulong)]
    return L


def parse(host, arg: bytes, lo: int = 0, hi: int = DEFAULT_L):
    """edges, or the diagnostic (str) of a rejection"""
    edges = (C.c_uint32 * 63)()
    err = C.create_string_buffer(200)
    n = host.pss_parse_length_edges(arg, lo, hi, edges, err, len(err))
    if n < 0:
        assert err.value, arg
        return err.value.decode()
    assert 1 <= n <= 63
    return list(edges[:n])


def tag(host, lo: int, hi: int) -> bytes:
    n = host.pss_length_bin_tag(lo, hi, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert host.pss_length_bin_tag(lo, hi, buf, n + 1) == n
    return buf.value


def test_parser_accepts_rising_edges(host):
    assert parse(host, b"30") == [30]
    assert parse(host, b"35,45,55,65") == [35, 45, 55, 65]
    assert parse(host, b"031,40") == [31, 40]                    # decimal, leading zeros are digits
    assert parse(host, b",".join(b"%d" % v for v in range(31, 94))) == list(range(31, 94))   # 63 edges
    # the extremes: l + 1 and L itself
    assert parse(host, b"11,80", lo=10, hi=80) == [11, 80]
    assert parse(host, b"1") == [1]
    assert parse(host, b"4294967295", hi=2 ** 40) == [2 ** 32 - 1]


@pytest.mark.parametrize("arg,lo,hi", [
    (b"", 0, DEFAULT_L),                       # empty list
    (b",", 0, DEFAULT_L),
    (b"30,", 0, DEFAULT_L),                    # empty item
    (b",30", 0, DEFAULT_L),
    (b"30,,40", 0, DEFAULT_L),
    (b"abc", 0, DEFAULT_L),                    # not a number
    (b"30,4x", 0, DEFAULT_L),
    (b"3.5", 0, DEFAULT_L),
    (b"-5", 0, DEFAULT_L),
    (b"+5", 0, DEFAULT_L),
    (b"0x20", 0, DEFAULT_L),
    (b" 30", 0, DEFAULT_L),                    # whitespace is not part of a decimal integer
    (b"30 ", 0, DEFAULT_L),
    (b"30, 40", 0, DEFAULT_L),
    (b"30\t", 0, DEFAULT_L),
    (b"30,30", 0, DEFAULT_L),                  # repeated
    (b"40,30", 0, DEFAULT_L),                  # decreasing
    (b"30,50,45", 0, DEFAULT_L),
    (b"0", 0, DEFAULT_L),                      # not above l
    (b"10", 10, DEFAULT_L),
    (b"5,20", 10, DEFAULT_L),
    (b"81", 0, 80),                            # above L
    (b"30,90", 0, 80),
    (b"4294967296", 0, 2 ** 40),               # above 2^32-1 whatever L is
    (b"99999999999999999999999", 0, 2 ** 40),
    (b",".join(b"%d" % v for v in range(31, 95)), 0, DEFAULT_L),   # 64 edges
])
def test_parser_rejects(host, arg, lo, hi):
    assert isinstance(parse(host, arg, lo, hi), str)


def test_parser_diagnostics_name_the_problem(host):
    assert "63" in parse(host, b",".join(b"%d" % v for v in range(31, 95)))
    assert "rise" in parse(host, b"30,30")
    assert "-l / -L" in parse(host, b"81", hi=80)
    assert "decimal" in parse(host, b"3a")


def test_bin_tags_and_bounds(host):
    assert tag(host, 0, 29) == b"len0-29"
    assert tag(host, 80, DEFAULT_L) == b"len80-250000000"
    assert tag(host, 2 ** 32 - 1, 2 ** 40) == b"len4294967295-1099511627776"
    buf = C.create_string_buffer(5)
    assert host.pss_length_bin_tag(30, 39, buf, 5) == 8 and buf.value == b"len3"
    edges = (C.c_uint32 * 3)(30, 40, 50)
    lo, hi = C.c_ulong(), C.c_ulong()
    got = []
    for b in range(4):
        host.pss_length_bin_bounds(edges, 3, b, 10, 80, C.byref(lo), C.byref(hi))
        got.append((lo.value, hi.value))
    assert got == [(10, 29), (30, 39), (40, 49), (50, 80)]


def test_length_bin_symbols_are_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    assert "pssbam_engine_set_length_bins" in pkg.HIP_SYMBOLS and hasattr(L, "pssbam_engine_set_length_bins")
    assert pkg.MAX_LENGTH_BINS == 64
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_MAX_LENGTH_BINS 64\b", hdr)
    assert re.search(r"int pssbam_engine_set_length_bins\(pssbam_engine \*e, int32_t n_edges, const uint32_t \*edges\);", hdr)
    edges = (C.c_uint32 * 1)(30)
    assert L.pssbam_engine_set_length_bins(None, 1, edges) == -1   # a NULL engine is refused, not touched
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_length_edges", "pss_length_bin_tag", "pss_length_bin_bounds"):
        assert hasattr(host, s)


def _run_cli(tmp_path, *args):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"),
                           *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args", [
    ["-S", ""], ["-S", "abc"], ["-S", "30,30"], ["-S", "40,30"], ["-S", "0"], ["-S", "30, 40"],
    ["-l", "30", "-S", "30"], ["-L", "80", "-S", "30,81"], ["-S", ",".join(str(v) for v in range(31, 95))],
])
def test_cli_refuses_bad_S_before_any_gpu_work(tmp_path, args):
    pr = _run_cli(tmp_path, *args)
    assert pr.returncode == 1
    assert "Unknown option -S" not in pr.stderr
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-S" in lines[0] and "Full command" not in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())


def test_cli_refuses_S_with_G_before_any_gpu_work(tmp_path):
    pr = _run_cli(tmp_path, "-S", "40", "-G")
    assert pr.returncode == 1
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-S" in lines[0] and "-G" in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())


def test_cli_knows_S(tmp_path):
    """-S takes an argument (the usage text is the reference's and stays as it is)"""
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-S", "40"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1
    assert "Unknown option" not in pr.stderr and pr.stderr.startswith("pss-bam v1.2.1:")

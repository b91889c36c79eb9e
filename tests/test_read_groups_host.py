"""pss-bam -G without a GPU: the @RG header parser and the ID -> file-name encoder of libpssbam_host.so,
the C-ABI symbols of libpssbam_hip.so, and the command line's -G / -R diagnostics."""
import ctypes as C
import re
import subprocess

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_read_groups.restype = C.c_int
    L.pss_parse_read_groups.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_char_p))]
    L.pss_free_read_groups.restype = None
    L.pss_free_read_groups.argtypes = [C.POINTER(C.c_char_p), C.c_int]
    L.pss_rg_file_tag.restype = C.c_size_t
    L.pss_rg_file_tag.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    return L


def parse(host, text: bytes) -> list[bytes]:
    ids = C.POINTER(C.c_char_p)()
    n = host.pss_parse_read_groups(text, len(text), C.byref(ids))
    assert n >= 0
    out = [ids[i] for i in range(n)]
    host.pss_free_read_groups(ids, n)
    return out


def tag(host, s: bytes) -> bytes:
    n = host.pss_rg_file_tag(s, None, 0)
    buf = C.create_string_buffer(n + 1)
    assert host.pss_rg_file_tag(s, buf, n + 1) == n
    return buf.value


def test_header_parser_order_duplicates_crlf_and_missing_ids(host):
    text = (b"@HD\tVN:1.6\n"
            b"@SQ\tSN:chr1\tLN:100\n"
            b"@RG\tID:libA\tSM:s1\n"
            b"@RG\tSM:s2\tLB:x\tID:libB\r\n"          # ID not the first tag, CRLF
            b"@RG\tSM:noid\n"                          # no ID: skipped
            b"@RG\tID:\tSM:empty\n"                    # empty ID: skipped
            b"@RG\tID:libA\tSM:again\n"                # duplicate: the first one counts
            b"@RGX\tID:notrg\n"                        # not an @RG line
            b"@CO\t@RG\tID:comment\n"
            b"@RG\tID:a/b\n@RG\tID:.\n@RG\tID:x%y\n"
            b"@RG\tID:last")                           # no final newline
    assert parse(host, text) == [b"libA", b"libB", b"a/b", b".", b"x%y", b"last"]


def test_header_parser_stops_at_nul_and_handles_empty(host):
    assert parse(host, b"") == []
    assert parse(host, b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:5\n") == []
    # a BAM header's l_text may include NUL padding
    assert parse(host, b"@RG\tID:g1\n\0\0@RG\tID:hidden\n") == [b"g1"]


def test_file_tag_encoder(host):
    assert tag(host, b"libA_1-x") == b"libA_1-x"
    assert tag(host, b"a/b") == b"a%2Fb"
    assert tag(host, b".") == b"%2E"
    assert tag(host, b"..") == b"%2E%2E"
    assert tag(host, b"x%y") == b"x%25y"
    assert tag(host, b"s p\xff") == b"s%20p%FF"
    # a short buffer is cut but NUL-terminated, and the full length is still reported
    buf = C.create_string_buffer(4)
    assert host.pss_rg_file_tag(b"a/b", buf, 4) == 5 and buf.value == b"a%2"


def test_read_group_symbols_are_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_read_groups", "pssbam_engine_finish_groups"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_MAX_READ_GROUPS 4096", hdr)
    # nothing has been counted and no engine exists: the calls refuse a NULL engine instead of touching it
    assert L.pssbam_engine_set_read_groups(None, 1, None) == -1
    assert L.pssbam_engine_finish_groups(None, 0, None, None) == -1


def test_cli_refuses_G_with_R_before_any_gpu_work(tmp_path):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"),
                         "-G", "-R", "x"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1
    assert "Unknown option -G" not in pr.stderr
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-G" in lines[0] and "-R" in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())


def test_cli_knows_G(tmp_path):
    """-G is an option of its own (the usage text is the reference's and stays as it is)"""
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-G"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1
    assert "Unknown option" not in pr.stderr and pr.stderr.startswith("pss-bam v1.2.1:")
    assert "-G" not in pr.stderr

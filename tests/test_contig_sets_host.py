"""pss-bam -C without a GPU: the contig -> set map parser of libpssbam_host.so, the C-ABI symbol of
libpssbam_hip.so, and the command line's -C diagnostics."""
import ctypes as C
import re
import subprocess

import pytest

import __graft_entry__ as ge


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_contig_sets.restype = C.c_int
    L.pss_parse_contig_sets.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_char_p)),
                                        C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_char_p)),
                                        C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.pss_free_contig_sets.restype = None
    L.pss_free_contig_sets.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.c_int]
    return L


def parse(host, text: bytes):
    """([(name, label)], [labels]), or the diagnostic (str) of a rejection"""
    names, set_of, labels = C.POINTER(C.c_char_p)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_char_p)()
    n_labels = C.c_int()
    err = C.create_string_buffer(600)
    n = host.pss_parse_contig_sets(text, len(text), C.byref(names), C.byref(set_of), C.byref(labels), C.byref(n_labels),
                                   err, len(err))
    if n < 0:
        assert err.value, text
        return err.value.decode()
    labs = [labels[i] for i in range(n_labels.value)]
    pairs = [(names[i], labs[set_of[i]]) for i in range(n)]
    host.pss_free_contig_sets(names, n, set_of, labels, n_labels.value)
    return pairs, labs


def test_parser_default_labels_comments_crlf_and_order(host):
    text = (b"# competitive mapping\n"
            b"chrM\tmt\n"
            b"\n"
            b"chrX  sex\r\n"                   # blanks of any kind, CRLF
            b"chrY sex\n"
            b"pathogen_1\n"                    # no label: the name itself
            b"   \t\n"                         # blank
            b"chrM mt\n"                       # the same name under the same label again: harmless
            b"#chrZ zzz\n"
            b"chr1\tauto somes\n"              # a label may hold blanks inside
            b"plasmid\tpathogen_1\n"
            b"last")                           # no final newline
    pairs, labs = parse(host, text)
    assert labs == [b"mt", b"sex", b"pathogen_1", b"auto somes", b"last"]
    assert pairs == [(b"chrM", b"mt"), (b"chrX", b"sex"), (b"chrY", b"sex"), (b"pathogen_1", b"pathogen_1"),
                     (b"chr1", b"auto somes"), (b"plasmid", b"pathogen_1"), (b"last", b"last")]
    assert parse(host, b"*\tunmapped\n") == ([(b"*", b"unmapped")], [b"unmapped"])


def test_parser_takes_many_names_and_4096_labels(host):
    pairs, labs = parse(host, b"".join(b"scaf%06d\tbin%d\n" % (i, i % 7) for i in range(120000)))
    assert len(pairs) == 120000 and labs == [b"bin%d" % i for i in range(7)]
    pairs, labs = parse(host, b"".join(b"c%d\n" % i for i in range(4096)))
    assert len(labs) == 4096


def test_parser_rejects_with_a_diagnostic(host):
    d = parse(host, b"chrX\tsex\nchrY\tsex\nchrM\tmt\nchrX mt\n")
    assert isinstance(d, str) and "chrX" in d and "two labels" in d and "line 1" in d and "line 4" in d
    for empty in (b"", b"\n\n", b"# only a comment\n  \n"):
        d = parse(host, empty)
        assert isinstance(d, str) and "no contig" in d
    d = parse(host, b"".join(b"c%d\n" % i for i in range(4097)))
    assert isinstance(d, str) and "4096" in d
    assert isinstance(parse(host, b"chrX\0\n"), str)


def test_contig_set_symbols_are_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    assert "pssbam_engine_set_contig_sets" in pkg.HIP_SYMBOLS and hasattr(L, "pssbam_engine_set_contig_sets")
    assert pkg.MAX_CONTIG_SETS == 4096
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_MAX_CONTIG_SETS 4096\b", hdr)
    assert re.search(r"int pssbam_engine_set_contig_sets\(pssbam_engine \*e, int32_t n_sets, int64_t n_names, "
                     r"const char \*const \*names,\s+const int32_t \*set_of\);", hdr)
    names, set_of = (C.c_char_p * 1)(b"chrX"), (C.c_int32 * 1)(0)
    assert L.pssbam_engine_set_contig_sets(None, 1, 1, names, set_of) == -1   # a NULL engine is refused, not touched
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_contig_sets", "pss_free_contig_sets", "pss_rg_file_tag"):
        assert hasattr(host, s)


def _run_cli(tmp_path, *args):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"),
                           *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("case", ["with_G", "with_S", "unreadable", "empty", "two_labels", "too_many", "directory"])
def test_cli_refuses_bad_C_before_any_gpu_work(tmp_path, case):
    maps = tmp_path / "maps"
    maps.mkdir()
    good = maps / "good.tsv"
    good.write_text("chrX\tsex\nchrY\tsex\n")
    args = {
        "with_G": ["-C", str(good), "-G"],
        "with_S": ["-C", str(good), "-S", "40"],
        "unreadable": ["-C", str(maps / "missing.tsv")],
        "empty": ["-C", str(maps / "empty.tsv")],
        "two_labels": ["-C", str(maps / "two.tsv")],
        "too_many": ["-C", str(maps / "many.tsv")],
        "directory": ["-C", str(maps)],
    }[case]
    (maps / "empty.tsv").write_text("# nothing\n\n")
    (maps / "two.tsv").write_text("chrX\tsex\nchrX\tauto\n")
    (maps / "many.tsv").write_text("".join(f"c{i}\n" for i in range(4097)))
    pr = _run_cli(tmp_path, *args)
    assert pr.returncode == 1
    assert "Unknown option -C" not in pr.stderr
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "-C" in lines[0] and "Full command" not in lines[0], pr.stderr
    if case in ("with_G", "with_S"):
        assert ("-G" if case == "with_G" else "-S") in lines[0]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["maps"]


def test_cli_knows_C(tmp_path):
    """-C takes an argument (the usage text is the reference's and stays as it is)"""
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-C", str(tmp_path / "m.tsv")], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1
    assert "Unknown option" not in pr.stderr and pr.stderr.startswith("pss-bam v1.2.1:")

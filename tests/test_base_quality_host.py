"""pss-bam -Q without a GPU: the C ABI carries the setter, the command line parses and refuses the option before any
GPU work, and the yardstick the GPU tests use -- the CPU oracle on a copy of the input with every base below q set to
N -- is itself checked against a direct count that skips those positions."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import pssbam_testlib as tl

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_pkg()


def test_setter_is_declared_listed_and_exported(pkg):
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^int pssbam_engine_set_min_base_quality\(pssbam_engine \*e, int32_t q\);$", hdr, re.M)
    assert "pssbam_engine_set_min_base_quality" in pkg.HIP_SYMBOLS
    L = pkg.hip_lib()
    f = L.pssbam_engine_set_min_base_quality
    f.argtypes = [C.c_void_p, C.c_int32]
    f.restype = C.c_int
    L.pssbam_last_error.restype = C.c_char_p
    assert f(None, 20) == -1                      # PSSBAM_EINVAL, not a dereference
    assert L.pssbam_last_error()


def test_abi_structs_keep_their_layout(pkg):
    """-Q adds an entry point, not a field: the option structs and the ABI version stay as they were"""
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    pss = hdr[hdr.index("typedef struct pssbam_pss_opts"):hdr.index("} pssbam_pss_opts;")]
    assert re.findall(r"(\w+);", pss) == ["region_len", "min_read_len", "max_read_len", "min_mq", "up_ctx", "down_ctx",
                                          "merged_only"]


BAD_Q = ["", "abc", "2x", "-1", "+5", " 20", "20 ", "94", "100", "4294967316", "2.5"]


@pytest.mark.parametrize("arg", BAD_Q)
def test_cli_refuses_bad_Q_before_any_work(pkg, arg, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    prefix = tmp_path / "out"
    pr = subprocess.run([str(exe), "-F", str(tmp_path / "no.fa"), "-B", str(tmp_path / "no.bam"), "-o", str(prefix), "-Q", arg],
                        capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    lines = pr.stderr.splitlines()
    assert len(lines) == 1 and "-Q" in lines[0], pr.stderr
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr
    assert pr.stdout == "" and list(tmp_path.iterdir()) == []


def test_cli_Q_alone_prints_the_usage(pkg):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    pr = subprocess.run([str(exe), "-Q", "20"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1
    assert pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr


def test_fragkon_has_no_Q(pkg):
    exe = pkg.PKG_DIR / "bin" / "fragkon"
    pr = subprocess.run([str(exe), "-Q", "20"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -Q." in pr.stderr


def test_host_parser_accepts_the_whole_range(pkg):
    L = C.CDLL(str(pkg.LIB_HOST))
    f = L.pss_parse_min_base_quality
    f.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    f.restype = C.c_int
    err = C.create_string_buffer(200)
    for q in (0, 1, 20, 41, 93, 7):
        assert f(str(q).encode(), err, 200) == q
    assert f(b"020", err, 200) == 20              # leading zeros are digits
    for bad in BAD_Q:
        assert f(bad.encode(), err, 200) == -1 and b"-Q" in err.value, bad


def test_masker_leaves_absent_fields_alone():
    assert bq.mask_seq("ACGT", "5555", 21) == "NNNN" and bq.mask_seq("ACGT", "5555", 20) == "ACGT"
    assert bq.mask_seq("ACGT", "!5+I", 11) == "NCNT"
    assert bq.mask_seq("*", "*", 40) == "*" and bq.mask_seq("ACGT", "*", 40) == "ACGT"
    assert bq.mask_seq("ACGT", "IIII", 0) == "ACGT"
    text = "@SQ\tSN:c\tLN:9\nr\t0\tc\t1\t9\t3M\t*\t0\t0\tACG\t!I!\tRG:Z:x\nq\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
    assert bq.mask_sam_text(text, 5) == text.replace("ACG", "NCN")


@pytest.mark.parametrize("q", [1, 20, 41, 42])
def test_oracle_on_masked_sam_equals_direct_count(oracle, tmp_path, q):
    """the yardstick: N-masking the SAM == leaving the low-quality positions out of the count"""
    contigs, refs, recs = tl.fuzz_dataset(8801, 3000)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        plain, masked = tmp_path / "plain.sam", tmp_path / "masked.sam"
        tl.write_sam(plain, refs, recs)
        bq.write_masked_sam(masked, refs, recs, q)
        for o in (tl.PssOpts(region_len=15), tl.PssOpts(region_len=31, min_mq=10, up_ctx="CT", down_ctx="ACGTN")):
            pf, pr_, pst = oracle.pss(g, plain, o)
            mf, mr, mst = oracle.pss(g, masked, o)
            df, dr = bq.direct_pss_counts(contigs, recs, o, q)
            assert np.array_equal(mf, df) and np.array_equal(mr, dr), (q, o)
            zf, zr = bq.direct_pss_counts(contigs, recs, o, 0)
            assert np.array_equal(pf, zf) and np.array_equal(pr_, zr), o      # (the direct count itself, unmasked)
            assert np.array_equal(pst, mst)                                   # no record changes its status
            assert np.array_equal(pf[:2], mf[:2]) and np.array_equal(pr_[:2], mr[:2])   # context rows: reference only
            if q > 2:   # the qualities run 2..41: from q = 3 on something is masked in both tables
                assert (pf[2:] != mf[2:]).any() and (pr_[2:] != mr[2:]).any()
            else:
                assert np.array_equal(pf, mf) and np.array_equal(pr_, mr)
    finally:
        oracle.free_genome(g)

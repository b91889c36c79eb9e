"""pss-bam -w (fixed windows: depth, GC content and the GC-bias table) without a GPU: the Python restatement of the definition
(windows_lib) against coverage_lib's own figures, the writer of libpssbam_host.so against the committed golden files, the bin
arithmetic on crafted arrays, the C-ABI symbol, and the command lines' refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import coverage_lib as cl
import windows_lib as wl


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    u64p, u32p, i32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    L.pss_write_windows.restype = C.c_int
    L.pss_write_windows.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int, C.POINTER(C.c_char_p), C.c_uint64, i32p, u32p, u32p, u32p, u32p,
                                    u32p, u64p]
    L.pss_gcbias_rows.restype = C.c_uint64
    L.pss_gcbias_rows.argtypes = [C.c_uint32, C.c_uint64, u32p, u32p, u32p, u32p, u64p, u64p, u64p]
    L.pss_parse_window.restype = C.c_int
    L.pss_parse_window.argtypes = [C.c_char_p, u32p]
    return L


def _arr(t, v):
    return (t * max(len(v), 1))(*[int(x) for x in v])


def write(host, prefix, refs, W, win, fasta=b"setD.fa", bam=b"setD.bam"):
    names = (C.c_char_p * len(refs))(*[nm.encode() for nm, _ in refs])
    return host.pss_write_windows(fasta, bam, str(prefix).encode(), W, len(refs), names, len(win[0]), _arr(C.c_int32, win[0]),
                                  *[_arr(C.c_uint32, v) for v in win[1:6]], _arr(C.c_uint64, win[6]))


def rows(host, W, start, end, acgt, gc, dsum):
    bw, bs = (C.c_uint64 * wl.GC_BINS)(), (C.c_uint64 * wl.GC_BINS)()
    used = host.pss_gcbias_rows(W, len(start), *[_arr(C.c_uint32, v) for v in (start, end, acgt, gc)], _arr(C.c_uint64, dsum), bw, bs)
    win = (np.zeros(len(start)), *(np.array(v, dtype=np.uint64) for v in (start, end, acgt, gc)), np.zeros(len(start)), np.array(dsum, dtype=np.uint64))
    assert (list(bw), list(bs), used) == wl.gcbias_rows(W, win)             # the C code and the restatement agree on every crafted case
    return {b: (int(bw[b]), int(bs[b])) for b in range(wl.GC_BINS) if bw[b]}, int(used)


# ---- the writers -----------------------------------------------------------------------------------------------------------------

def test_writer_matches_the_golden_files(host, tmp_path):
    refs, seqs, spans = wl.golden()
    W = wl.GOLDEN_W
    win = wl.from_spans(spans, refs, seqs, W)
    size = win[2].astype(int) - win[1].astype(int)
    bw, _, used = wl.gcbias_rows(W, win)
    assert (size == W).any() and (size < W).any() and 0 < used < len(size) and sum(1 for n in bw if n) >= 3
    assert write(host, tmp_path / "out", refs, W, win) == 0
    got_w, got_g = (tmp_path / "out.pss.windows.txt").read_bytes(), (tmp_path / "out.pss.gcbias.txt").read_bytes()
    assert got_w == (cl.GOLD / "windows_setD.windows.txt").read_bytes() and got_w.decode() == wl.windows_text("setD.fa", "setD.bam", refs, W, win)
    assert got_g == (cl.GOLD / "windows_setD.gcbias.txt").read_bytes() and got_g.decode() == wl.gcbias_text("setD.fa", "setD.bam", W, win)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.gcbias.txt", "out.pss.windows.txt"]            # (no .tmp stays)


def test_writer_na_large_counts_empty_and_unwritable_prefix(host, tmp_path):
    refs = [("c", 2 ** 31), ("gone", 5), ("e", 40)]
    W = 2 ** 30
    win = (np.array([0, 0, 2], dtype=np.int32), np.array([0, W, 0], dtype=np.uint32), np.array([W, 2 ** 31, 40], dtype=np.uint32),
           np.array([W, 2 ** 29, 0], dtype=np.uint32), np.array([2 ** 29, 2 ** 29, 0], dtype=np.uint32), np.array([W, 7, 0], dtype=np.uint32),
           np.array([2 ** 50, 2 ** 40 + 1, 0], dtype=np.uint64))
    assert write(host, tmp_path / "o", refs, W, win, b"f", b"b") == 0
    text = (tmp_path / "o.pss.windows.txt").read_text()
    assert text == wl.windows_text("f", "b", refs, W, win)
    assert text.splitlines()[6:] == [f"c\t0\t{W}\t{W}\t{2 ** 29}\t0.500000\t{W}\t{2 ** 50}\t1048576.000000",
                                     f"c\t{W}\t{2 ** 31}\t{2 ** 29}\t{2 ** 29}\t1.000000\t7\t{2 ** 40 + 1}\t1024.000000", "e\t0\t40\t0\t0\tNA\t0\t0\t0.000000"]
    bias = (tmp_path / "o.pss.gcbias.txt").read_text()
    assert bias == wl.gcbias_text("f", "b", W, win)
    assert "# used windows: 2\n" in bias and f"50\t1\t{W}\t{2 ** 50}\t1048576.000000\t" in bias and f"100\t1\t{W}\t{2 ** 40 + 1}\t1024.000000\t" in bias
    # no window at all is two files
    none = tuple(np.zeros(0, dtype=dt) for dt in wl.DTYPES)
    assert write(host, tmp_path / "empty", refs, 16, none) == 0
    assert (tmp_path / "empty.pss.windows.txt").read_text() == wl.windows_text("setD.fa", "setD.bam", refs, 16, none)
    assert (tmp_path / "empty.pss.gcbias.txt").read_text() == wl.gcbias_text("setD.fa", "setD.bam", 16, none)
    # an unwritable place, a window outside the names, and a name taken by a directory leave nothing behind
    assert write(host, tmp_path / "no_such_dir" / "o", refs, W, win) == 1
    bad = (np.array([0, 7, 2], dtype=np.int32),) + win[1:]
    assert write(host, tmp_path / "bad", refs, W, bad) == 1
    (tmp_path / "dir.pss.gcbias.txt").mkdir()
    assert write(host, tmp_path / "dir", refs, W, win) == 1
    assert sorted(p.name for p in tmp_path.iterdir()) == ["dir.pss.gcbias.txt", "empty.pss.gcbias.txt", "empty.pss.windows.txt", "o.pss.gcbias.txt",
                                                          "o.pss.windows.txt"]
    assert not list((tmp_path / "dir.pss.gcbias.txt").iterdir())


# ---- the identities ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [16, 17, 100, "longest", 2 ** 30])
def test_windows_sum_to_the_contigs_lines_of_c(W):
    refs, seqs, spans = wl.golden()
    lens = {n: len(s) for n, s in seqs.items()}
    W = max(lens.values()) if W == "longest" else W
    depths = cl.depth_arrays(spans, refs, lens)
    s = cl.summarise(depths)
    ref, start, end, acgt, gc, covered, dsum = wl.windows(depths, refs, seqs, W)
    assert [v.dtype for v in (ref, start, end, acgt, gc, covered, dsum)] == [np.dtype(t) for t in wl.DTYPES]
    at = 0
    for i, (n, _) in enumerate(refs):
        sel = np.flatnonzero(ref == i)
        n_w = -(-lens[n] // W)
        assert np.array_equal(sel, np.arange(at, at + n_w))                                      # by refID, then start, nothing else
        at += n_w
        assert np.array_equal(start[sel], np.arange(n_w) * W) and np.array_equal(end[sel], np.minimum((np.arange(n_w) + 1) * W, lens[n]))
        assert int(covered[sel].sum()) == int(s.per_contig[i][0]) and int(dsum[sel].sum()) == int(s.per_contig[i][1])
        if W >= lens[n]:                                                                         # one window: the contig's line itself
            assert n_w == 1 and (int(end[sel][0]), int(covered[sel][0]), int(dsum[sel][0])) == (lens[n], int(s.per_contig[i][0]), int(s.per_contig[i][1]))
        for k in sel:                                                                            # ... and the depth array's own sums
            d = depths[i][int(start[k]):int(end[k])]
            letters = seqs[n][int(start[k]):int(end[k])].upper()
            assert int(dsum[k]) == int(d.sum()) and int(covered[k]) == int((d > 0).sum())
            assert int(acgt[k]) == sum(letters.count(c) for c in "ACGT") and int(gc[k]) == letters.count("C") + letters.count("G")
    assert at == len(ref)


def test_lower_case_n_and_iupac_letters_and_a_reference_the_genome_lacks():
    refs = [("b", 40), ("ghost", 99), ("a", 20), ("b", 40)]
    seqs = {"a": "acgtNNRYacgtACGTnnnn", "b": "C" * 16 + "g" * 8 + "K" * 8 + "ATat" + "SW-*", "extra": "ACGT"}
    win = wl.from_spans([(0, 2, 30), (2, 0, 20), (2, 5, 3)], refs, seqs, 16)
    assert [v.tolist() for v in win] == [[0, 0, 0, 2, 2], [0, 16, 32, 0, 16], [16, 32, 40, 16, 20], [16, 8, 4, 12, 0], [16, 8, 0, 6, 0],
                                         [14, 16, 0, 16, 4], [14, 16, 0, 19, 4]]


# ---- the bin arithmetic ----------------------------------------------------------------------------------------------------------

def test_gc_bins_on_crafted_windows(host):
    W = 101
    # acgt = 0; 2 acgt = W - 1 (left out) and, with an even W below, = W (used)
    assert rows(host, W, [0, 101], [101, 202], [0, 50], [0, 25], [5, 7]) == ({}, 0)
    assert rows(host, 100, [0, 100], [100, 200], [49, 50], [10, 25], [5, 7]) == ({50: (1, 7)}, 1)
    assert rows(host, W, [0], [101], [51], [51], [9]) == ({100: (1, 9)}, 1)
    # gc / acgt at x.5 % exactly rounds up: 1/200 -> 1, 25/200 -> 13, 199/200 -> 100, 99/200 -> 50; 98/200 is 49 % exactly
    assert rows(host, 200, [0] * 5, [200] * 5, [200] * 5, [1, 25, 199, 99, 98], [1, 2, 3, 4, 5]) == ({1: (1, 1), 13: (1, 2), 100: (1, 3), 50: (1, 4), 49: (1, 5)}, 5)
    assert rows(host, 16, [0, 0, 0], [16, 16, 16], [16, 8, 8], [0, 8, 4], [0, 0, 2 ** 40]) == ({0: (1, 0), 100: (1, 0), 50: (1, 2 ** 40)}, 3)
    # a short last window is left out, whatever it holds; several windows share a bin
    assert rows(host, 16, [0, 16, 32], [16, 32, 47], [16, 16, 15], [8, 8, 15], [3, 4, 100]) == ({50: (2, 7)}, 2)
    # no used window at all: every row is zero, and so are the means
    assert rows(host, 16, [0], [5], [5], [5], [50]) == ({}, 0) and rows(host, 16, [], [], [], [], []) == ({}, 0)
    win = (np.zeros(1, dtype=np.int32), *(np.array([v], dtype=np.uint32) for v in (0, 5, 5, 5, 5)), np.array([50], dtype=np.uint64))
    text = wl.gcbias_text("f", "b", 16, win)
    assert "# used windows: 0\n# mean depth of the used windows: 0.000000\n" in text
    assert text.splitlines()[8:] == ["%d\t0\t0\t0\t0.000000\t0.000000" % b for b in range(101)]


def test_window_size_parser(host):
    v = C.c_uint32(0)
    for good in ("16", "17", "1000", str(2 ** 30), "0064"):
        assert host.pss_parse_window(good.encode(), C.byref(v)) == 0 and v.value == int(good)
    for bad in ("", "15", "0", "-16", "+16", "16.0", "1e3", "16k", " 16", "16 ", str(2 ** 30 + 1), str(2 ** 32 + 16), "9" * 30, "x"):
        assert host.pss_parse_window(bad.encode(), C.byref(v)) == 1, bad


# ---- the C ABI and the command lines ---------------------------------------------------------------------------------------------

def test_windows_symbol_is_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    s = "pssbam_engine_finish_coverage_windows"
    assert s in pkg.HIP_SYMBOLS and hasattr(L, s) and hasattr(pkg.Engine, "finish_coverage_windows")
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"int pssbam_engine_finish_coverage_windows\(pssbam_engine \*e, uint32_t window, uint64_t cap, int32_t \*ref, uint32_t \*start, "
                     r"uint32_t \*end,\s+uint32_t \*acgt, uint32_t \*gc, uint32_t \*covered, uint64_t \*depth_sum, uint64_t \*n_windows\);", hdr)
    assert re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert L.pssbam_engine_finish_coverage_windows(None, 100, 0, None, None, None, None, None, None, None, None) == -1   # a NULL engine is refused, not touched


def _run_cli(tool, tmp_path, *args, env=None):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / tool
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"), *args],
                          capture_output=True, text=True, timeout=60, env={**os.environ, **(env or {})})


def _one_line(pr, tmp_path):
    assert pr.returncode == 1
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "Unknown option" not in pr.stderr and "Full command" not in lines[0], pr.stderr
    assert not list(tmp_path.iterdir())
    return lines[0]


@pytest.mark.parametrize("size", ["15", "0", "-5", "100.5", "1e6", "64k", "", str(2 ** 30 + 1), str(2 ** 32 + 64)])
def test_cli_refuses_a_size_that_is_no_whole_number_in_range(tmp_path, size):
    line = _one_line(_run_cli("pss-bam", tmp_path, "-w", size), tmp_path)
    assert "-w takes a window size" in line and f"16..{2 ** 30}" in line


@pytest.mark.parametrize("args", [["-w", "100", "-I"], ["-I", "-w", "100"]])
def test_cli_refuses_w_with_I_before_any_work(tmp_path, args):
    line = _one_line(_run_cli("pss-bam", tmp_path, *args), tmp_path)
    assert "-w" in line and "-I" in line and "does not go with" in line


def test_cli_refuses_w_on_several_gpus_before_any_work(tmp_path):
    line = _one_line(_run_cli("pss-bam", tmp_path, "-w", "100", env={"PSSBAM_NGPU": "2"}), tmp_path)
    assert "-w" in line and "PSSBAM_NGPU=2" in line


def test_fragkon_has_no_w(tmp_path):
    line = _one_line(_run_cli("fragkon", tmp_path, "-w", "100"), tmp_path)
    assert "-w" in line and "pss-bam" in line and "fragkon has none" in line


def test_cli_knows_w():
    pkg = ge.load_pkg()
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-w", "100"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "Unknown option" not in pr.stderr and "-w <size> <also write" in pr.stderr

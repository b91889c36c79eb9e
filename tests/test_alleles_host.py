"""Allele counts of the tallied reads at listed sites (pss-bam -a / -t) without a GPU: the Python restatement of the definition
(alleles_lib) against a brute-force loop and against coverage_lib's depth, the sites-file reader and the report writer of
libpssbam_host.so against the restatement and the committed golden files, the stand-alone hostcheck driver, the C-ABI symbols, and
the command lines' refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import alleles_lib as al
import coverage_lib as cl
import duplicates_lib as dl
import pssbam_testlib as tl


class _Sites(C.Structure):
    _fields_ = [("n_names", C.c_int32), ("names", C.POINTER(C.c_char_p)), ("n", C.c_int64), ("name_of", C.POINTER(C.c_int32)), ("pos0", C.POINTER(C.c_uint32))]


@pytest.fixture(scope="module")
def host():
    pkg = ge.load_pkg()
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_sites.restype = C.c_int
    L.pss_parse_sites.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(_Sites), C.c_char_p, C.c_size_t]
    L.pss_read_sites.restype = C.c_int
    L.pss_read_sites.argtypes = [C.c_char_p, C.POINTER(_Sites), C.c_char_p, C.c_size_t]
    L.pss_free_sites.argtypes = [C.POINTER(_Sites)]
    L.pss_write_alleles.restype = C.c_int
    L.pss_write_alleles.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(C.c_int32),
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    return L


def c_parse(host, data: bytes, path=b"x.sites"):
    """-> [(contig, pos0)], or the reader's message"""
    st, err = _Sites(), C.create_string_buffer(600)
    rc = host.pss_parse_sites(path, data, len(data), C.byref(st), err, len(err))
    if rc:
        assert st.n == 0 and not st.names
        return err.value.decode()
    out = [(st.names[st.name_of[i]].decode(), int(st.pos0[i])) for i in range(st.n)]
    host.pss_free_sites(C.byref(st))
    return out


def c_write(host, prefix, refs, res, bases, counts, fasta=b"setD.fa", bam=b"setD.bam", sites=b"alleles_setD.sites", trim=0):
    n, m = len(refs), int(res.ref.size)
    names = (C.c_char_p * n)(*[nm.encode() for nm, _ in refs])
    arr = lambda t, v: (t * max(len(v), 1))(*[int(x) for x in v])  # noqa: E731
    t = al.totals(res, counts)
    return host.pss_write_alleles(fasta, bam, sites, trim, str(prefix).encode(), n, names, m, arr(C.c_int32, res.ref), arr(C.c_uint32, res.pos0),
                                  arr(C.c_uint8, bases), arr(C.c_uint32, counts.reshape(-1)), arr(C.c_uint64, [t["given"], t["resolved"], t["covered"], t["bases"]]))


def fuzz_kept(seed, n, **pss):
    """(refs, seqs, raw records) of a fuzz set's records that the candidate test keeps -- N and IUPAC letters, mixed qualities, both
    strands, pairs among them"""
    contigs, refs, recs = tl.fuzz_dataset(seed, n)
    s = dl.Setup(refs, {nm: len(q) for nm, q in contigs}, pss=tl.PssOpts(**pss))
    idx = {nm: i for i, (nm, _) in enumerate(refs)}
    keep = [r for r in recs if cl.kept(cl.core_of_rec(r, idx), s)]
    return refs, dict(contigs), dl.split_raw(tl.raw_records(refs, keep))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("trim,min_bq", [(0, 0), (1, 0), (3, 20), (0, 30), (40, 0)])
def test_restatement_equals_a_loop_over_every_base_of_every_read(trim, min_bq):
    refs, seqs, raws = fuzz_kept(7301, 700, region_len=6, min_mq=10)
    reads = [al.read_of_raw(b) for b in raws]
    assert len(reads) > 100 and any(r.rev for r in reads) and any(not r.rev for r in reads)
    rng = np.random.default_rng(trim * 100 + min_bq)
    contigs = {n: len(q) for n, q in seqs.items()}
    sites = [(n, int(p)) for n, ln in contigs.items() for p in rng.integers(0, ln + 20, size=max(ln // 6, 4))] + [("absent", 3)]
    res = al.resolve(sites, refs, contigs)
    got, want = al.count(reads, res, refs, trim, min_bq), al.count_brute(reads, res, refs, trim, min_bq)
    assert np.array_equal(got, want) and got.dtype == np.uint32
    assert res.given == len(set(sites)) > res.ref.size > 0
    assert np.array_equal(np.lexsort((res.pos0, res.ref)), np.arange(res.ref.size))
    if trim < 40:
        assert int(got.sum()) > 0 and int(got[:, [4, 9]].sum()) > 0           # something lands on "other"
    if trim == 0 and min_bq == 0:
        assert all(int(got[:, k].sum()) > 0 for k in range(10))


def test_the_ten_counters_sum_to_the_depth_at_the_site_on_setD():
    refs, seqs, reads = al.golden_reads()
    contigs = {n: len(q) for n, q in seqs.items()}
    _, _, spans = cl.kept_of_golden()
    assert len(spans) == len(reads)
    depth = cl.depth_arrays(spans, refs, contigs)
    res = al.resolve(al.golden_sites(refs, seqs), refs, contigs)
    counts = al.count(reads, res, refs)
    sums = counts.astype(np.int64).sum(axis=1)
    want = np.array([depth[int(r)][int(p)] for r, p in zip(res.ref, res.pos0)])
    assert np.array_equal(sums, want) and int(sums.max()) >= 3 and int((sums == 0).sum()) > 0
    trimmed = al.count(reads, res, refs, trim=2).astype(np.int64).sum(axis=1)
    assert np.all(trimmed <= sums) and int(trimmed.sum()) < int(sums.sum())


def test_every_position_as_a_site_gives_the_base_composition_of_the_kept_reads():
    refs, seqs, raws = fuzz_kept(7302, 500, region_len=4)
    reads = [al.read_of_raw(b) for b in raws]
    contigs = {n: len(q) for n, q in seqs.items()}
    res = al.resolve([(n, p) for n, ln in contigs.items() for p in range(ln)], refs, contigs)
    assert res.ref.size == sum(contigs[n] for n in {n for n, _ in refs} if n in contigs)
    counts = al.count(reads, res, refs)
    want = np.zeros(10, dtype=np.int64)
    for r in reads:
        codes = np.full(r.L, 4, dtype=np.int64)
        m = min(r.L, r.nib.size)
        codes[:m] = al.CODE_OF_NIBBLE[r.nib[:m]]
        want += np.roll(np.concatenate([np.bincount(codes, minlength=5), np.zeros(5, dtype=np.int64)]), 5 if r.rev else 0)
    assert np.array_equal(counts.astype(np.int64).sum(axis=0), want) and want.min() > 0
    bases = al.ref_bases(res, refs, seqs)
    assert set(bytes(bases)) <= set(b"ACGTN") and bases.size == res.ref.size


# ---- the sites file ----------------------------------------------------------------------------------------------------------------

GOOD = (b"# a comment\n"
        b"chr1\t752566\trs1\tA\tG\n"
        b"\n"
        b"chr1 10   extra columns  are ignored\r\n"
        b"  chr2\t1\n"
        b"#chr9\t5\n"
        b"chr1\t752566\n"
        b"\tchrUn_x\t4294967296")


def test_reader_takes_extra_columns_comments_crlf_and_a_last_line_without_a_newline(host):
    want = [("chr1", 752565), ("chr1", 9), ("chr2", 0), ("chr1", 752565), ("chrUn_x", 2 ** 32 - 1)]
    assert c_parse(host, GOOD) == want == al.parse_sites(GOOD.decode())
    many = "".join(f"c{k % 150}\t{k + 1}\n" for k in range(5000)).encode()      # more names and sites than the first allocations hold
    assert c_parse(host, many) == al.parse_sites(many.decode()) == [(f"c{k % 150}", k) for k in range(5000)]


@pytest.mark.parametrize("data,line,what", [
    (b"chr1\t5\nchr1\n", 2, "two fields"),
    (b"chr1\t5\n\n# c\nchr1\tx7\n", 4, "not a decimal integer"),
    (b"chr1\t-5\n", 1, "not a decimal integer"),
    (b"chr1\t5.0\n", 1, "not a decimal integer"),
    (b"chr1\t0\n", 1, "1-based"),
    (b"chr1\t1\r\nchr1\t4294967297\r\n", 2, "at most 2^32"),
    (b"chr1\t99999999999999999999999\n", 1, "at most 2^32"),
    (b"chr1   \n", 1, "two fields"),
])
def test_reader_names_the_file_and_the_line_of_a_malformed_line(host, data, line, what):
    msg = c_parse(host, data, path=b"panel/my.sites")
    assert isinstance(msg, str) and msg.startswith("-a: panel/my.sites: ") and f"line {line}:" in msg and what in msg, msg
    with pytest.raises(ValueError, match=f"line {line}:"):
        al.parse_sites(data.decode())


def test_reader_refuses_an_empty_a_missing_and_a_compressed_file(host, tmp_path):
    for data in (b"", b"# only\n\n  \n"):
        msg = c_parse(host, data)
        assert isinstance(msg, str) and "holds no site" in msg
        with pytest.raises(ValueError):
            al.parse_sites(data.decode())
    st, err = _Sites(), C.create_string_buffer(600)
    assert host.pss_read_sites(str(tmp_path / "none.txt").encode(), C.byref(st), err, len(err)) == -1 and b"unable to read" in err.value
    import gzip
    (tmp_path / "s.gz").write_bytes(gzip.compress(b"chr1\t5\n"))
    assert host.pss_read_sites(str(tmp_path / "s.gz").encode(), C.byref(st), err, len(err)) == -1 and b"compressed" in err.value
    (tmp_path / "s.txt").write_bytes(GOOD)
    assert host.pss_read_sites(str(tmp_path / "s.txt").encode(), C.byref(st), err, len(err)) == 0 and st.n == 5 and st.n_names == 3
    host.pss_free_sites(C.byref(st))


# ---- the writer and the golden -----------------------------------------------------------------------------------------------------

def test_golden_regenerates_byte_for_byte_and_the_writer_writes_it(host, tmp_path):
    sites_text, report = al.golden_text()
    assert sites_text.encode() == (al.GOLD / "alleles_setD.sites").read_bytes()
    assert report.encode() == (al.GOLD / "alleles_setD.txt").read_bytes()
    refs, seqs, reads = al.golden_reads()
    contigs = {n: len(q) for n, q in seqs.items()}
    sites = c_parse(host, (al.GOLD / "alleles_setD.sites").read_bytes())
    assert sites == al.golden_sites(refs, seqs)
    res = al.resolve(sites, refs, contigs)
    counts = al.count(reads, res, refs)
    assert res.given == len(sites) - 1 and res.ref.size == res.given - 2          # one duplicate; one ghost contig, one beyond the end
    assert c_write(host, tmp_path / "out", refs, res, al.ref_bases(res, refs, seqs), counts) == 0
    assert (tmp_path / "out.pss.alleles.txt").read_bytes() == report.encode()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.pss.alleles.txt"]      # (no .tmp stays)
    lines = report.splitlines()
    assert lines[2] == "#contig\tpos\tref\tfA\tfC\tfG\tfT\tfO\trA\trC\trG\trT\trO" and len(lines) == 3 + res.ref.size
    assert any(ln.split("\t")[3:] == ["0"] * 10 for ln in lines[3:])                  # depth 0 has a line too


def test_writer_large_counts_no_site_and_what_it_refuses(host, tmp_path):
    refs = [("c", 2 ** 32), ("gone", 5)]
    res = al.Resolved(np.array([0, 0], dtype=np.int32), np.array([0, 2 ** 32 - 1], dtype=np.uint32), 3, {}, {})
    counts = np.array([[2 ** 32 - 1] * 10, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]], dtype=np.uint32)
    assert c_write(host, tmp_path / "o", refs, res, np.frombuffer(b"NA", dtype=np.uint8), counts, b"f", b"b", b"s", trim=65535) == 0
    assert (tmp_path / "o.pss.alleles.txt").read_text().splitlines() == [
        "# pss-bam allele counts  fasta f bam b sites s  trim 65535",
        f"# sites_given 3 sites_resolved 2 sites_covered 2 bases_counted {10 * (2 ** 32 - 1) + 45}",
        "#contig\tpos\tref\tfA\tfC\tfG\tfT\tfO\trA\trC\trG\trT\trO",
        "c\t1\tN" + f"\t{2 ** 32 - 1}" * 10, f"c\t{2 ** 32}\tA\t0\t1\t2\t3\t4\t5\t6\t7\t8\t9"]
    none = al.Resolved(np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint32), 4, {}, {})
    assert c_write(host, tmp_path / "e", refs, none, np.zeros(0, dtype=np.uint8), np.zeros((0, 10), dtype=np.uint32)) == 0
    assert len((tmp_path / "e.pss.alleles.txt").read_text().splitlines()) == 3
    assert c_write(host, tmp_path / "no_such_dir" / "o", refs, res, np.frombuffer(b"NA", dtype=np.uint8), counts) == 1
    bad = al.Resolved(np.array([0, 2], dtype=np.int32), res.pos0, 3, {}, {})                 # a reference the list lacks
    assert c_write(host, tmp_path / "bad", refs, bad, np.frombuffer(b"NA", dtype=np.uint8), counts) == 1
    assert sorted(p.name for p in tmp_path.iterdir()) == ["e.pss.alleles.txt", "o.pss.alleles.txt"]


def test_hostcheck_driver_reads_and_writes(tmp_path):
    pkg = ge.load_pkg()
    hc = pkg.PKG_DIR / "bin" / "hostcheck"
    good = tmp_path / "good.sites"
    good.write_bytes(GOOD)
    pr = subprocess.run([str(hc), "-s", str(good), "-S", str(tmp_path / "hc")], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 0 and pr.stdout.startswith("sites names=3 sites=5 digest="), pr.stdout + pr.stderr
    lines = (tmp_path / "hc.pss.alleles.txt").read_text().splitlines()
    assert len(lines) == 3 + 5 and lines[3].startswith("chr1\t752566\tA\t") and lines[7].startswith("chrUn_x\t4294967296\tN\t")
    assert not (tmp_path / "hc.pss.alleles.txt.tmp").exists()
    same = subprocess.run([str(hc), "-s", str(al.GOLD / "alleles_setD.sites")], capture_output=True, text=True, timeout=60)
    assert same.returncode == 0 and re.match(r"sites names=\d+ sites=\d+ digest=[0-9a-f]{16}\n$", same.stdout)
    for data in (b"chr1\t5\nchr1\n", b"chr1\t0\n", b"", b"chr1\tfive\n"):
        bad = tmp_path / "bad.sites"
        bad.write_bytes(data)
        pr = subprocess.run([str(hc), "-s", str(bad), "-S", str(tmp_path / "never")], capture_output=True, text=True, timeout=60)
        assert pr.returncode == 1 and pr.stderr.startswith("hostcheck: -a: ") and str(bad) in pr.stderr
    assert not list(tmp_path.glob("never*"))


def test_hostcheck_driver_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the stand-alone driver of `make sanitize`, instrumented: the reader and the writer over good and bad files, silently"""
    pkg = ge.load_pkg()
    pr = subprocess.run(["make", "-s", "-C", str(pkg.PKG_DIR), "bin/san/hostcheck.asan"], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-3000:]
    hc, plain = pkg.PKG_DIR / "bin" / "san" / "hostcheck.asan", pkg.PKG_DIR / "bin" / "hostcheck"
    env = {**os.environ, "ASAN_OPTIONS": "detect_leaks=1 exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1 halt_on_error=1"}
    many = tmp_path / "many.sites"
    many.write_text("".join(f"c{k % 150}\t{k + 1}\textra\r\n" for k in range(5000)))
    good = tmp_path / "good.sites"
    good.write_bytes(GOOD)
    for k, f in enumerate((good, many, al.GOLD / "alleles_setD.sites")):
        got = subprocess.run([str(hc), "-s", str(f), "-S", str(tmp_path / f"san{k}")], capture_output=True, text=True, timeout=120, env=env)
        want = subprocess.run([str(plain), "-s", str(f), "-S", str(tmp_path / f"plain{k}")], capture_output=True, text=True, timeout=120)
        assert got.returncode == 0 and "Sanitizer" not in got.stderr and "runtime error" not in got.stderr, got.stderr[-3000:]
        assert got.stdout == want.stdout and got.stdout.startswith("sites names=")
        a, b = (tmp_path / f"san{k}.pss.alleles.txt").read_text(), (tmp_path / f"plain{k}.pss.alleles.txt").read_text()
        assert a == b and len(a.splitlines()) > 3
    for data in (b"chr1\t5\nchr1\n", b"chr1\t0", b"", b"#\n", b"chr1\t99999999999999999999999999999999\n", b"c" * 70000, b"\tchr1\t \t \n"):
        bad = tmp_path / "bad.sites"
        bad.write_bytes(data)
        pr = subprocess.run([str(hc), "-s", str(bad)], capture_output=True, text=True, timeout=120, env=env)
        assert pr.returncode == 1 and pr.stderr.startswith("hostcheck: -a: ") and "Sanitizer" not in pr.stderr and "runtime error" not in pr.stderr, pr.stderr[-3000:]


# ---- the C ABI and the command lines ---------------------------------------------------------------------------------------------

def test_site_symbols_are_exported():
    pkg = ge.load_pkg()
    L = pkg.hip_lib()
    for s in ("pssbam_engine_set_sites", "pssbam_engine_finish_sites"):
        assert s in pkg.HIP_SYMBOLS and hasattr(L, s)
    assert pkg.MAX_SITE_TRIM == al.MAX_TRIM == 65535
    hdr = (pkg.ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"#define PSSBAM_MAX_SITE_TRIM 65535\b", hdr) and re.search(r"#define PSSBAM_ABI_VERSION 1\b", hdr)
    assert re.search(r"int pssbam_engine_set_sites\(pssbam_engine \*e, int32_t n_names, const char \*const \*names, int64_t n_sites, const int32_t \*name_of,\s+"
                     r"const uint32_t \*pos0, uint32_t trim\);", hdr)
    assert re.search(r"int pssbam_engine_finish_sites\(pssbam_engine \*e, uint64_t cap, int32_t \*ref, uint32_t \*pos0, uint8_t \*ref_base,\s+uint32_t \*counts "
                     r"/\* 10 per site: fA fC fG fT fO rA rC rG rT rO \*/, uint64_t \*n_sites, uint64_t totals\[4\]\);", hdr)
    assert L.pssbam_engine_set_sites(None, 0, None, 0, None, None, 0) == -1      # a NULL engine is refused, not touched
    assert L.pssbam_engine_finish_sites(None, 0, None, None, None, None, None, None) == -1


def _run_cli(tool, tmp_path, *args, env=None):
    pkg = ge.load_pkg()
    exe = pkg.PKG_DIR / "bin" / tool
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"), *args],
                          capture_output=True, text=True, timeout=60, env={**os.environ, **(env or {})})


def _one_line(pr, tmp_path, left=()):
    assert pr.returncode == 1
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1 and "Unknown option" not in pr.stderr and "Full command" not in lines[0], pr.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(left)
    return lines[0]


@pytest.mark.parametrize("args", [["-a", "s.txt", "-I"], ["-I", "-t", "2", "-a", "s.txt"]])
def test_cli_refuses_sites_with_I_before_any_work(tmp_path, args):
    line = _one_line(_run_cli("pss-bam", tmp_path, *args), tmp_path)
    assert "-a" in line and "-I" in line and "does not go with" in line


def test_cli_refuses_t_alone_and_t_out_of_range(tmp_path):
    assert "needs -a" in _one_line(_run_cli("pss-bam", tmp_path, "-t", "2"), tmp_path)
    for v in ("-1", "65536", "x", "3x", ""):
        line = _one_line(_run_cli("pss-bam", tmp_path, "-a", "s.txt", "-t", v), tmp_path)
        assert "-t takes a number of bases in 0..65535" in line


def test_cli_refuses_sites_on_several_gpus_and_a_malformed_file_before_any_work(tmp_path):
    line = _one_line(_run_cli("pss-bam", tmp_path, "-a", "s.txt", env={"PSSBAM_NGPU": "2"}), tmp_path)
    assert "-a" in line and "PSSBAM_NGPU=2" in line
    bad = tmp_path / "bad.sites"
    bad.write_bytes(b"chr1\t5\nchr1\tfive\n")
    line = _one_line(_run_cli("pss-bam", tmp_path, "-a", str(bad)), tmp_path, left=["bad.sites"])
    assert line == f"-a: {bad}: line 2: the position is not a decimal integer"
    line = _one_line(_run_cli("pss-bam", tmp_path, "-a", str(tmp_path / "missing.sites")), tmp_path, left=["bad.sites"])
    assert "unable to read" in line


@pytest.mark.parametrize("args", [["-a", "s.txt"], ["-t", "2"]])
def test_fragkon_has_neither(tmp_path, args):
    line = _one_line(_run_cli("fragkon", tmp_path, *args), tmp_path)
    assert args[0] in line and "pss-bam" in line


def test_cli_knows_a_and_t():
    pkg = ge.load_pkg()
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-a", "s.txt", "-t", "1"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and "Unknown option" not in pr.stderr
    assert "-a <sites.txt>" in pr.stderr and "-t <n> <with -a" in pr.stderr

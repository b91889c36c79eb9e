"""pss-bam -J without a GPU: the read-name hash in C against its Python restatement and the published vectors, the -J
parser, the jackknife in C against numpy, the writer of the standard-error file, the command line's refusals, and the
golden the unmodified reference wrote for setA reduced to replicate 1 of 3."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl
import replicates_lib as rp

ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


@pytest.fixture(scope="module")
def host(pkg):
    L = C.CDLL(str(pkg.LIB_HOST))
    L.pss_parse_replicates.restype = C.c_int
    L.pss_parse_replicates.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.pss_read_name_hash.restype = C.c_uint32
    L.pss_read_name_hash.argtypes = [C.c_char_p, C.c_size_t]
    L.pss_read_name_replicate.restype = C.c_int
    L.pss_read_name_replicate.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
    L.pss_jackknife_se.restype = C.c_int
    L.pss_jackknife_se.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pss_write_rates_se.restype = C.c_int
    L.pss_write_rates_se.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


# ---- the hash ----------------------------------------------------------------------------------------------------------

def test_vectors(host):
    for name, h in rp.VECTORS.items():
        assert rp.name_hash(name) == h and host.pss_read_name_hash(name, len(name)) == h, name


def hash_names():
    rng = np.random.default_rng(41)
    names = [bytes(rng.integers(1, 128, size=n, dtype=np.uint8)) for n in list(range(10)) + [253, 254] for _ in range(4)]
    stem = b"lib7:0042:1101:"                                   # 15 bytes, then tails of 1..4 bytes that differ in their last byte only
    for n_tail in (1, 2, 3, 4):
        names += [stem + b"x" * (n_tail - 1) + bytes([c]) for c in (0x30, 0x31, 0x7E)]
    names += [b"ab\0cd", b"ab\0ce", b"ab\0", b"ab", b"\0", b"\0\0\0\0", b"\0\0\0\0\0"]      # embedded and trailing NULs count
    names += [bytes([0x80, 0xFF, 0xC3, 0xA9]), bytes([0xFF] * 7), b"r\xe9ad/1", bytes(range(0x80, 0x100))]
    return names


@pytest.mark.parametrize("k", [2, 3, 20, 64])
def test_c_hash_is_the_python_hash(host, k):
    names = hash_names()
    assert {len(n) for n in names} >= set(range(10)) | {253, 254}
    for name in names:
        assert host.pss_read_name_hash(name, len(name)) == rp.name_hash(name), name
        j = host.pss_read_name_replicate(name, len(name), k)
        assert j == rp.replicate(name, k) and 0 <= j < k, name
    # the tail bytes, the length and the NULs all reach the hash
    assert len({rp.name_hash(n) for n in names}) == len(set(names))


def test_fixture_spread():
    """the figures the GPU tests and the golden rely on"""
    names = [ln.split("\t", 1)[0] for ln in (GOLD / "setA.sam").read_text().splitlines() if not ln.startswith("@")]
    assert np.bincount([rp.replicate(n, 3) for n in names]).tolist() == [228, 227, 224]
    per = np.bincount([rp.replicate(f"r{i:07d}", 20) for i in range(1500)], minlength=20)
    assert (int(per.min()), int(per.max())) == (54, 85)


# ---- the parser --------------------------------------------------------------------------------------------------------

def parse(host, arg: bytes):
    err = C.create_string_buffer(200)
    v = host.pss_parse_replicates(arg, err, len(err))
    if v < 0:
        assert v == -1 and err.value and b"\n" not in err.value, arg
        return err.value.decode()
    return v


@pytest.mark.parametrize("arg,want", [(b"2", 2), (b"5", 5), (b"64", 64), (b"020", 20)])
def test_parser_accepts(host, arg, want):
    assert parse(host, arg) == want


@pytest.mark.parametrize("arg", [b"1", b"0", b"65", b"x", b"", b"-3", b"+5", b" 5", b"5 ", b"3.5", b"0x10", b"99999999999999999999"])
def test_parser_rejects_with_a_message(host, arg):
    msg = parse(host, arg)
    assert isinstance(msg, str) and "-J" in msg and "2..64" in msg
    assert "at least 2" in parse(host, b"1") and "above 64" in parse(host, b"65") and "decimal" in parse(host, b"x")


# ---- the jackknife -----------------------------------------------------------------------------------------------------

def random_planes(rng, n: int, k: int, empty_pos=None):
    """K replicate tables that really differ: each replicate has its own substitution rate"""
    planes = np.zeros((k, n + 2, 16), dtype=np.uint64)
    for j in range(k):
        depth = int(rng.integers(200, 400))
        p_sub = 0.01 + 0.05 * rng.random()
        for row in range(n + 2):
            for ref in range(4):
                tot = int(rng.integers(depth // 2, depth))
                subs = rng.multinomial(tot, [p_sub / 3] * 3 + [1 - p_sub])
                others = [b for b in range(4) if b != ref]
                for b, c in zip(others + [ref], subs):
                    planes[j, row, 4 * b + ref] = c
    if empty_pos is not None:                                   # reference base G was never seen at this position
        planes[:, empty_pos + 2, 2::4] = 0
    return planes


def c_jackknife(host, total, planes):
    k, rows = planes.shape[0], planes.shape[1]
    total, planes = np.ascontiguousarray(total, dtype=np.uint64), np.ascontiguousarray(planes, dtype=np.uint64)
    out = np.full((rows - 2, 12), -1.0)
    assert host.pss_jackknife_se(rows - 2, k, total.ctypes.data, planes.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("n,k,empty", [(15, 2, None), (15, 5, 3), (40, 20, 0), (7, 64, 6), (1, 3, None)])
def test_jackknife_against_numpy(host, n, k, empty):
    """absolute 1e-12: rates are <= 1 and at most 64 terms are summed in double, a rounding error of the order 64 * 2.2e-16"""
    rng = np.random.default_rng(1000 * n + k)
    planes = random_planes(rng, n, k, empty)
    total = planes.sum(axis=0)
    want, got = rp.jackknife_se(total, planes), c_jackknife(host, total, planes)
    print(f"n={n} k={k}: max |C - numpy| = {np.abs(got - want).max():.3e}, max SE = {want.max():.3e}")
    assert np.abs(got - want).max() <= 1e-12
    assert want.max() > 1e-6 and (want >= 0).all()
    if empty is not None:
        assert not got[empty].any() and not want[empty].any()   # an empty reference column: twelve zeros in every theta_j
        assert got[[p for p in range(n) if p != empty]].min() > 0


def test_jackknife_by_hand(host):
    """K = 2, one position: theta_0 and theta_1 are each other replicate's rate, SE = |theta_0 - theta_1| / 2"""
    planes = np.zeros((2, 3, 16), dtype=np.uint64)
    for j, (ct, cc) in enumerate(((3, 97), (10, 90))):           # read T on reference C: cell 13; read C on C: cell 5
        planes[j, 2, [0, 10, 15]] = 50
        planes[j, 2, 13], planes[j, 2, 5] = ct, cc
    got = c_jackknife(host, planes.sum(axis=0), planes)
    want = np.zeros(12)
    want[rp.OFF_DIAG.index(13)] = abs(0.10 - 0.03) / 2
    assert np.abs(got[0] - want).max() <= 1e-15
    same = np.stack([planes[0], planes[0]])
    assert not c_jackknife(host, same.sum(axis=0), same).any()  # identical replicates: an exact 0


# ---- the writer --------------------------------------------------------------------------------------------------------

def test_writer(host, tmp_path):
    n, k = 4, 7
    fwd = np.arange(n * 12, dtype=np.float64).reshape(n, 12) * 1.25e-4
    rev = fwd[::-1].copy() + 0.5
    fwd[1, 3] = 0.0
    prefix = tmp_path / "out"
    assert host.pss_write_rates_se(b"the genome.fa", b"in.bam", str(prefix).encode(), n, k, fwd.ctypes.data, rev.ctypes.data) == 0
    assert [p.name for p in tmp_path.iterdir()] == ["out.pss.rates.se.txt"]
    text = (tmp_path / "out.pss.rates.se.txt").read_text()
    head, blocks = rp.parse_rates_text(text)
    assert head == ["### pss-bam.c v1.2.1", "### FASTA: the genome.fa", "### BAM: in.bam", f"### OUT: {prefix}.pss.rates.se.txt",
                    "### Format of table:",
                    "### Substitution rates for all possible nucleotide substitutions at",
                    "### each position in the aligned reads.",
                    "### First base is what was seen in the read.",
                    "### Second base is what was in the genome at that position.",
                    "### POS AC AG AT CA CG CT GA GC GT TA TC TG",
                    "### jackknife standard errors of the forward read substitution rates, K = 7 read-name replicates",
                    "### jackknife standard errors of the reverse read substitution rates, K = 7 read-name replicates"]
    (lab_f, val_f), (lab_r, val_r) = blocks
    assert lab_f == [0, 1, 2, 3] and lab_r == [3, 2, 1, 0]
    assert val_f == [[f"{x:.5e}" for x in row] for row in fwd] and val_r == [[f"{x:.5e}" for x in row] for row in rev[::-1]]
    assert val_f[1][3] == "0.00000e+00"
    assert "\n\n\n### jackknife standard errors of the reverse" in text   # two blank lines between the blocks
    # the layout of the rates file itself: same lines but OUT and the two captions
    rates = np.zeros((n, 12))
    lib = C.CDLL(str(ge.load_pkg().LIB_HOST))
    lib.pss_write_rates.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.pss_write_rates(b"the genome.fa", b"in.bam", str(prefix).encode(), n, rates.ctypes.data, rates.ctypes.data) == 0
    rhead, rblocks = rp.parse_rates_text((tmp_path / "out.pss.rates.txt").read_text())
    assert [a == b for a, b in zip(head, rhead)] == [True] * 3 + [False] + [True] * 6 + [False] * 2
    assert [b[0] for b in rblocks] == [lab_f, lab_r]
    assert host.pss_write_rates_se(b"f", b"b", str(tmp_path / "no_such_dir" / "o").encode(), n, k, fwd.ctypes.data, rev.ctypes.data) == 1


# ---- symbols -----------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_listed_and_exported(pkg):
    L = pkg.hip_lib()
    assert "pssbam_engine_set_replicates" in pkg.HIP_SYMBOLS and hasattr(L, "pssbam_engine_set_replicates")
    assert pkg.MAX_REPLICATES == 64
    hdr = (ROOT / "include" / "pssbam_hip.h").read_text()
    assert re.search(r"^#define PSSBAM_MAX_REPLICATES 64\b", hdr, re.M)
    assert re.search(r"^int pssbam_engine_set_replicates\(pssbam_engine \*e, int32_t k\);$", hdr, re.M)
    assert L.pssbam_engine_set_replicates(None, 5) == -1            # a NULL engine is refused, not touched
    for name in ("set_replicates", "finish_replicates", "replicates"):
        assert hasattr(pkg.Engine, name)
    host = C.CDLL(str(pkg.LIB_HOST))
    for s in ("pss_parse_replicates", "pss_read_name_replicate", "pss_jackknife_se", "pss_write_rates_se"):
        assert hasattr(host, s)


# ---- the command line --------------------------------------------------------------------------------------------------

def _run_cli(pkg, tmp_path, *args):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(tmp_path / "none.fa"), "-B", str(tmp_path / "none.bam"), "-o", str(tmp_path / "o"),
                           *args], capture_output=True, text=True, timeout=60)


def _one_line(pr, tmp_path):
    assert pr.returncode == 1, (pr.returncode, pr.stderr)
    assert "Unknown option" not in pr.stderr and "Full command" not in pr.stderr
    lines = pr.stderr.strip().splitlines()
    assert len(lines) == 1, pr.stderr
    assert pr.stdout == "" and not list(tmp_path.iterdir())
    return lines[0]


OTHERS = [(["-G"], "-G"), (["-S", "40"], "-S"), (["-C", "no_such_map.tsv"], "-C"), (["-H", "100"], "-H"), (["-X", "cpg"], "-X"),
          (["-E", "ss"], "-E"), (["-I"], "-I"), (["-A"], "-A"), (["-n", "1"], "-n"), (["-N", "4"], "-N"), (["-V"], "-V")]


@pytest.mark.parametrize("other,word", OTHERS)
def test_cli_refuses_each_excluded_option(pkg, tmp_path, other, word):
    for args in (["-J", "5"] + other, other + ["-J", "5"]):
        line = _one_line(_run_cli(pkg, tmp_path, *args), tmp_path)
        assert line.startswith("-J (jackknife replicates) and ") and word in line and line.endswith(" exclude each other.")


@pytest.mark.parametrize("arg,word", [("1", "at least 2"), ("65", "above 64"), ("x", "decimal"), ("", "needs")])
def test_cli_refuses_bad_counts_with_the_parsers_message(pkg, host, tmp_path, arg, word):
    line = _one_line(_run_cli(pkg, tmp_path, "-J", arg), tmp_path)
    assert line == parse(host, arg.encode()) and word in line


def test_cli_usage_names_the_option_and_fragkon_has_none(pkg):
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "pss-bam"), "-J", "5"], capture_output=True, text=True, timeout=60)
    assert pr.returncode == 1 and pr.stderr.startswith("pss-bam v1.2.1") and "Unknown option" not in pr.stderr
    assert len([ln for ln in pr.stderr.splitlines() if ln.startswith("-J <K>")]) == 1
    pr = subprocess.run([str(pkg.PKG_DIR / "bin" / "fragkon"), "-J", "5"], capture_output=True, text=True, timeout=60)
    assert "Unknown option -J." in pr.stderr


# ---- golden ------------------------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


def test_golden(oracle, tmp_path):
    """tests/golden/rep1of3_setA.pss.{counts,rates}.txt are what the unmodified reference wrote for setA.sam reduced to
    replicate 1 of 3 (tests/golden/make_replicates_golden.py); the oracle on the same reduced text reproduces them"""
    text = (GOLD / "setA.sam").read_text()
    reduced = tmp_path / "setA.rep1of3_setA.sam"
    reduced.write_text(rp.reduce_sam_text(text, 3, 1))
    assert sum(not ln.startswith("@") for ln in reduced.read_text().splitlines()) == 227
    g = oracle.load_genome(GOLD / "setA.fa")
    try:
        fwd, rev, _ = oracle.pss(g, reduced, tl.PssOpts())
        full_f, full_r, _ = oracle.pss(g, GOLD / "setA.sam", tl.PssOpts())
        parts = [oracle.pss(g, _write(tmp_path / f"p{j}.sam", rp.reduce_sam_text(text, 3, j)), tl.PssOpts()) for j in range(3)]
    finally:
        oracle.free_genome(g)
    wf, wr = tl.parse_counts_text((GOLD / "rep1of3_setA.pss.counts.txt").read_text())
    assert np.array_equal(fwd, wf) and np.array_equal(rev, wr)
    assert wf[2:].sum() > 0 and wf.sum() < full_f.sum()
    # the three reductions partition the input
    assert np.array_equal(sum(p[0] for p in parts), full_f) and np.array_equal(sum(p[1] for p in parts), full_r)
    oracle.write_reports("setA.fa", "x.sam", str(tmp_path / "orc"), fwd, rev)
    for kind in ("counts", "rates"):
        assert report_body((tmp_path / f"orc.pss.{kind}.txt").read_text()) == report_body((GOLD / f"rep1of3_setA.pss.{kind}.txt").read_text()), kind


def _write(path: Path, text: str) -> Path:
    path.write_text(text)
    return path


def test_reduce_matches_the_sam_text_reduction():
    contigs, refs, recs = tl.fuzz_dataset(11, 300, extras=True)
    text = "".join(tl.sam_line(r) for r in recs)
    for k, j in ((2, 0), (5, 3), (20, 19)):
        assert rp.reduce_sam_text(text, k, j) == "".join(tl.sam_line(r) for r in rp.reduce(recs, k, j))
    assert sum(len(rp.reduce(recs, 7, j)) for j in range(7)) == len(recs)

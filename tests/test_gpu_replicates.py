"""pss-bam -J on the GPU: K read-name replicates, one plane each, picked by a hash of the read name in the tally kernels.
The yardstick is the engine WITHOUT the setting on the input reduced to one replicate (replicates_lib.reduce, the hash
restated in Python): every replicate's tables must equal it exactly, the totals and the status counters must not move,
and plane 0 stays empty.  The subset-equality test also compares with the CPU oracle on the reduced SAM text."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import mismatch_lib as ml
import pssbam_testlib as tl
import regions_lib as rl
import replicates_lib as rp

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
SEED = 7401     # every replicate of K = 2, 5, 7, 20 has a non-empty forward table at -r 15 and -r 40 (the least: 248 counts)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq,
                up_ctx=o.up_ctx, down_ctx=o.down_ctx, merged_only=o.merged_only)


def kern_of(pkg, name: str) -> int:
    return pkg.KERNEL_TILED if name == "TILED" else pkg.KERNEL_SIMPLE


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, regions=None, **kw):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, **kw)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if regions is not None:
        eng.set_regions(*rl.to_arrays(regions))
    if recs:
        eng.submit(tl.raw_records(refs, recs))
    return eng


def tables_of(pkg, contigs, refs, recs, o, kernel, **kw):
    eng = run_engine(pkg, contigs, refs, recs, o, kernel, **kw)
    tot = eng.finish()
    eng.close()
    return tot


def zero_group(eng) -> bool:
    fwd = np.ones((eng.region_len + 2, 16), dtype=np.uint64)
    rev = np.ones_like(fwd)
    assert eng._L.pssbam_engine_finish_groups(eng._h, -1, fwd.ctypes.data, rev.ctypes.data) == 0
    return not fwd.any() and not rev.any()


def check_replicates(pkg, contigs, refs, recs, o, kernel, k, oracle_case=None, **kw):
    """every replicate against the engine without the setting on its reduction; totals, status counters, plane 0, the sum"""
    eng = run_engine(pkg, contigs, refs, recs, o, kernel, replicates=k, **kw)
    assert eng.replicates == k
    fwd, rev = eng.finish_replicates()
    tot = eng.finish()
    assert zero_group(eng)
    eng.close()
    assert fwd.shape == rev.shape == (k, o.region_len + 2, 16) and fwd.dtype == np.uint64
    plain = tables_of(pkg, contigs, refs, recs, o, kernel, **kw)
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev) and tot.stats == plain.stats
    assert np.array_equal(fwd.sum(axis=0), tot.fwd) and np.array_equal(rev.sum(axis=0), tot.rev)
    for j in range(k):
        part = rp.reduce(recs, k, j)
        want = tables_of(pkg, contigs, refs, part, o, kernel, **kw)
        assert want.fwd.any(), (k, j)                              # the condition: nothing is compared with an empty table
        assert np.array_equal(fwd[j], want.fwd) and np.array_equal(rev[j], want.rev), (k, j)
        if oracle_case is not None:
            orc, g, tmp = oracle_case
            sam = tmp / f"k{k}_j{j}.sam"
            tl.write_sam(sam, refs, part)
            of, orv, _ = orc.pss(g, sam, o)
            assert np.array_equal(fwd[j], of) and np.array_equal(rev[j], orv), (k, j)
    return fwd, rev, tot


@pytest.fixture(scope="module")
def fuzz():
    return tl.fuzz_dataset(SEED, 1500, extras=True)               # names r%07d, some padded to 254 bytes


# ---- subset equality ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("n", [15, 40])
@pytest.mark.parametrize("k", [2, 5, 7, 20])
def test_subset_equality(pkg, oracle, fuzz, tmp_path, kernel, n, k):
    """-r 40 takes a second row pass; the larger K take more than one plane pass where the staged prefixes leave less
    room for planes (test_forced_plane_passes pins that path)"""
    contigs, refs, recs = fuzz
    assert max(len(r.qname) for r in recs) == 254 and sum(len(r.qname) > 200 for r in recs) > 20
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        check_replicates(pkg, contigs, refs, recs, tl.PssOpts(region_len=n), kern_of(pkg, kernel), k, oracle_case=(oracle, g, tmp_path))
    finally:
        oracle.free_genome(g)


# ---- forced plane passes, several tiles per workgroup, the one-lane path ---------------------------------------------

@pytest.mark.parametrize("n", [15, 40])
def test_forced_plane_passes(pkg, fuzz, monkeypatch, n):
    """PSSBAM_GROUP_SLOTS=2: the six planes of K = 5 take three plane passes (times two row passes at -r 40)"""
    monkeypatch.setenv("PSSBAM_GROUP_SLOTS", "2")
    check_replicates(pkg, *fuzz, tl.PssOpts(region_len=n), pkg.KERNEL_TILED, 5)


def test_several_tiles_per_workgroup(pkg, monkeypatch):
    """PSSBAM_TILE_READS=64 and few workgroups: a workgroup walks several tiles, the staging buffer is refilled under the hash"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_GRID_WGS", "3")
    contigs, refs, recs = tl.fuzz_dataset(SEED + 1, 3000, extras=True)
    check_replicates(pkg, contigs, refs, recs, tl.PssOpts(region_len=15), pkg.KERNEL_TILED, 5)


def test_one_lane_path(pkg, fuzz, monkeypatch):
    """a staged prefix of 5 pieces does not hold a long-name record through QUAL[0]: it is hashed from global memory"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    _, _, tot = check_replicates(pkg, *fuzz, tl.PssOpts(region_len=15), pkg.KERNEL_TILED, 5)
    assert tot.stats["slow_path"] > 0


# ---- crafted names -------------------------------------------------------------------------------------------------------

def crafted_names() -> list:
    rng = np.random.default_rng(77)
    rand = lambda n: bytes(rng.integers(33, 127, size=n, dtype=np.uint8))   # noqa: E731
    names = [rand(n) for n in (0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 254)]
    for n in (1, 2, 3, 5, 6, 7, 9, 10, 11, 33, 34, 35, 253, 254):           # equal in the first 4 * (n // 4) bytes, different in the tail
        stem, n_tail = rand(4 * (n // 4)), n - 4 * (n // 4)
        if n_tail == 0:
            continue
        tail = rand(n_tail)
        names += [stem + tail, stem + tail[:-1] + bytes([tail[-1] ^ 1]), stem + bytes([tail[0] ^ 2]) + tail[1:]]
    names += [b"ab\0cd", b"ab\0ce", bytes([0x80, 0xFF, 0xC3]), bytes([0xFF] * 9)]   # an embedded NUL, bytes >= 0x80
    names = list(dict.fromkeys(names))
    while len(names) < 64:
        nm = rand(int(rng.integers(10, 40)))
        if nm not in names:
            names.append(nm)
    assert len(names) == 64
    return names


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_crafted_names(pkg, kernel):
    """64 identical <40>M reads that pass every filter, under crafted names: each record lands in the plane Python names,
    one at a time and together, with the names starting at all four byte alignments of the block"""
    kern = kern_of(pkg, kernel)
    ctg = ml.clean_contig(2000)
    contigs, refs = [("clean", ctg)], [("clean", len(ctg))]
    names = crafted_names()
    raw = [rp.raw_record(nm, 0, 100, ctg[100:140]) for nm in names]
    o = tl.PssOpts(region_len=15)
    unit_eng = run_engine(pkg, contigs, refs, [], o, kern)
    unit_eng.submit(np.frombuffer(raw[20], dtype=np.uint8))
    unit = unit_eng.finish()
    unit_eng.close()
    assert unit.stats["pss_ok"] == 1 and unit.fwd.sum() == unit.rev.sum() == 17
    for k in (5, 64):
        eng = run_engine(pkg, contigs, refs, [], o, kern, replicates=k)
        for nm, rec in zip(names, raw):                               # one at a time
            eng.reset()
            eng.submit(np.frombuffer(rec, dtype=np.uint8))
            fwd, rev = eng.finish_replicates()
            j = rp.replicate(nm, k)
            assert np.array_equal(fwd[j], unit.fwd) and np.array_equal(rev[j], unit.rev), (nm, k)
            assert fwd.sum() == rev.sum() == 17, (nm, k)              # and nowhere else
        for shift in range(4):                                        # together; rotating the list moves every name's alignment
            order = names[shift:] + names[:shift]
            block = b"".join(rp.raw_record(nm, 0, 100, ctg[100:140]) for nm in order)
            starts = np.cumsum([0] + [len(rp.raw_record(nm, 0, 100, ctg[100:140])) for nm in order])[:-1]
            assert {int(s + 36) & 3 for s in starts} == {0, 1, 2, 3}
            eng.reset()
            eng.submit(np.frombuffer(block, dtype=np.uint8))
            fwd, rev = eng.finish_replicates()
            per = np.bincount([rp.replicate(nm, k) for nm in order], minlength=k)
            for j in range(k):
                assert np.array_equal(fwd[j], unit.fwd * np.uint64(per[j])) and np.array_equal(rev[j], unit.rev * np.uint64(per[j])), (k, j, shift)
            assert eng.finish().stats["pss_ok"] == 64
        eng.close()


# ---- with the other settings ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_a_read_group(pkg, kernel):
    contigs, refs, recs = tl.fuzz_dataset(SEED + 2, 1500, with_rg=True)
    _, _, tot = check_replicates(pkg, contigs, refs, recs, tl.PssOpts(region_len=15), kern_of(pkg, kernel), 5, read_group="grpA")
    assert tot.stats["rg_dropped"] > 300


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_a_minimum_base_quality(pkg, fuzz, kernel):
    o = tl.PssOpts(region_len=15)
    _, _, tot = check_replicates(pkg, *fuzz, o, kern_of(pkg, kernel), 5, min_base_qual=20)
    assert not np.array_equal(tot.fwd, tables_of(pkg, *fuzz, o, kern_of(pkg, kernel)).fwd)     # the mask did bite


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_regions(pkg, kernel):
    contigs, refs, recs, ivs = rl.fuzz_case(rl.PSS_SEEDS[0])
    o = tl.PssOpts(region_len=15)
    _, _, tot = check_replicates(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), 5, regions=ivs)
    all_ok = tables_of(pkg, contigs, refs, recs, o, kern_of(pkg, kernel)).stats["pss_ok"]
    assert 0.25 * all_ok < tot.stats["pss_ok"] < 0.75 * all_ok                                  # about half the reads


# ---- the feed, a bound counter block -------------------------------------------------------------------------------------

def test_submit_bgzf_replicates_set_after_feed_open(pkg, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(SEED + 3, 4000, extras=True)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    o = tl.PssOpts(region_len=15, min_mq=5)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_replicates(5)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    fwd, rev = eng.finish_replicates()
    tot = eng.finish()
    assert eng.feed_status()["flags"] == 0 and tot.stats["records"] == len(recs)
    eng.close()
    plain = tables_of(pkg, contigs, refs, recs, o, pkg.KERNEL_TILED)
    assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev)
    for j in range(5):
        want = tables_of(pkg, contigs, refs, rp.reduce(recs, 5, j), o, pkg.KERNEL_TILED)
        assert want.fwd.any() and np.array_equal(fwd[j], want.fwd) and np.array_equal(rev[j], want.rev), j


def test_two_engines_share_a_bound_block(pkg, fuzz):
    """two engines bound to one block of the reported size give the sum, at the offsets counter_layout() documents; read
    back raw, as a caller that sums blocks across GPUs would see it"""
    contigs, refs, recs = fuzz
    o, k = tl.PssOpts(region_len=15), 5
    owner = pkg.Engine(pss=pss_dict(o), replicates=k)
    lay = owner.counter_layout()
    d, n = owner.counters_device()
    assert n == lay["n_u64"]
    owner.sync()                                                    # the block is zeroed
    engs = []
    for _ in range(2):                                              # binding carries the engine's own (empty) block over: both bind first
        eng = pkg.Engine(pss=pss_dict(o), replicates=k)
        eng.bind_counters(d, n)
        assert eng.counters_device() == (d, n)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        eng.sync()
        engs.append(eng)
    for eng, part in zip(engs, (recs[:700], recs[700:])):
        eng.submit(tl.raw_records(refs, part))
    for eng in engs:
        eng.sync()
    fwd, rev = engs[0].finish_replicates()
    host = np.zeros(n, dtype=np.uint64)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(host.ctypes.data, d, host.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    for eng in engs + [owner]:
        eng.close()
    cells = (o.region_len + 2) * 16
    assert not host[:lay["stats"]].any()                            # plane 0 stays empty
    assert int(host[lay["stats"] + pkg.ST_NAMES.index("records")]) == len(recs)
    for j in range(k):
        want = tables_of(pkg, contigs, refs, rp.reduce(recs, k, j), o, pkg.KERNEL_TILED)
        at = lay["replicates"][j]
        assert at["replicate"] == j and at["rev"] == at["fwd"] + cells
        assert np.array_equal(host[at["fwd"]:at["fwd"] + cells].reshape(-1, 16), want.fwd)
        assert np.array_equal(host[at["rev"]:at["rev"] + cells].reshape(-1, 16), want.rev)
        assert np.array_equal(fwd[j], want.fwd) and np.array_equal(rev[j], want.rev)


# ---- rules ---------------------------------------------------------------------------------------------------------------

OTHER_SETTINGS = [("read_groups", dict(read_groups=["a"]), "set_read_groups", (["a"],)),
                  ("length_bins", dict(length_bins=[30]), "set_length_bins", ([30],)),
                  ("contig_sets", dict(contig_sets={"x": ["chrA"]}), "set_contig_sets", ({"x": ["chrA"]},)),
                  ("per_contig", dict(per_contig=True), "set_per_contig", (True,)),
                  ("length_hist", dict(length_hist=100), "set_length_histogram", (100,)),
                  ("site_context", dict(site_context="cpg"), "set_site_context", ("cpg",)),
                  ("end_condition", dict(end_condition=(1, 13, 13)), "set_end_condition", (1, 13, 13)),
                  ("gapped", dict(gapped=True), "set_gapped", (True,)),
                  ("mismatches", dict(mismatches=(4, -1, 0)), "set_mismatches", (4, -1, 0)),
                  ("mismatch filter", dict(mismatches=(0, 2, 0)), "set_mismatches", (0, 2, 0))]


@pytest.mark.parametrize("what,ctor,setter,args", OTHER_SETTINGS, ids=[s[0] for s in OTHER_SETTINGS])
def test_rules_exclusions_both_ways(pkg, what, ctor, setter, args):
    E = pkg.PssbamError
    eng = pkg.Engine(pss=dict(region_len=5), **ctor)
    n_before = eng.counters_device()[1]
    with pytest.raises(E, match=r"replicates and .* exclude each other"):
        eng.set_replicates(5)
    assert eng.replicates == 0 and eng.counters_device()[1] == n_before
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), replicates=5)
    n_before = eng.counters_device()[1]
    with pytest.raises(E, match=r"and replicates exclude each other"):
        getattr(eng, setter)(*args)
    assert eng.replicates == 5 and eng.counters_device()[1] == n_before
    eng.close()


def test_rules(pkg, fuzz):
    E = pkg.PssbamError
    for bad in (1, -1, 65, 1 << 20):
        with pytest.raises(E):
            pkg.Engine(pss=dict(region_len=5), replicates=bad)
    with pytest.raises(E):                                          # k-mer replicates are out of scope
        pkg.Engine(kmer=dict(klen=4), replicates=5)
    with pytest.raises(E):                                          # and so is the mixed mask
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), replicates=5)
    for k in (2, 64):
        eng = pkg.Engine(pss=dict(region_len=5), replicates=k)
        assert eng.replicates == k
        eng.close()

    contigs, refs, recs = fuzz
    recs = recs[:400]
    o = tl.PssOpts(region_len=5)
    plain = tables_of(pkg, contigs, refs, recs, o, pkg.KERNEL_TILED)
    eng = pkg.Engine(pss=pss_dict(o), read_group=None, min_base_qual=0, replicates=5)
    lay = eng.counter_layout()
    base = lay["stats"] + pkg.ST_N
    assert [r["fwd"] for r in lay["replicates"]] == [base + j * 2 * 7 * 16 for j in range(5)]
    assert [r["rev"] for r in lay["replicates"]] == [base + j * 2 * 7 * 16 + 7 * 16 for j in range(5)]
    assert lay["n_u64"] == base + 5 * 2 * 7 * 16 == eng.counters_device()[1]
    eng.set_replicates(7)                                           # another count before the first tally
    assert eng.counter_layout()["n_u64"] == base + 7 * 2 * 7 * 16 == eng.counters_device()[1]
    eng.set_replicates(0)                                           # off: the block and the kernels of a plain engine
    assert eng.replicates == 0 and "replicates" not in eng.counter_layout()
    assert eng.counter_layout()["n_u64"] == base == eng.counters_device()[1]
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    got = eng.finish()
    assert np.array_equal(got.fwd, plain.fwd) and np.array_equal(got.rev, plain.rev) and got.stats == plain.stats
    with pytest.raises(E):                                          # no planes
        eng.finish_replicates()
    for k in (0, 5):
        with pytest.raises(E, match="tallied"):                     # records have been tallied
            eng.set_replicates(k)
    eng.reset()
    eng.set_replicates(5)                                           # legal again after reset
    eng.submit(tl.raw_records(refs, recs))
    first = eng.finish_replicates()
    assert first[0].any()
    with pytest.raises(E, match="tallied"):
        eng.set_replicates(6)
    eng.reset()                                                     # the setting survives reset
    assert eng.replicates == 5 and eng.counters_device()[1] == base + 5 * 2 * 7 * 16
    zf, zr = eng.finish_replicates()
    assert not zf.any() and not zr.any()
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_replicates()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    eng.close()

    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E, match="bound"):                           # a bound counter block cannot grow
        eng.set_replicates(5)
    eng.close()
    other.close()


# ---- the command line ----------------------------------------------------------------------------------------------------

CLI_MODES = {
    "bam_device_feed": ("bam", {}),
    "bam_host_reader": ("bam", {"PSSBAM_DEVICE_INFLATE": "0"}),
    "sam": ("sam", {}),
    "bam_two_gpus": ("bam", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}),
}
CLI_K = 5


@pytest.fixture(scope="module")
def cli_case(pkg):
    """the records, and the numpy jackknife of Engine.finish_replicates() over them"""
    contigs, refs, recs = tl.fuzz_dataset(SEED + 4, 4000)
    recs = tl.ref_safe(recs)
    o = tl.PssOpts(region_len=25, min_mq=10)
    eng = run_engine(pkg, contigs, refs, recs, o, pkg.KERNEL_AUTO, replicates=CLI_K)
    fwd, rev = eng.finish_replicates()
    tot = eng.finish()
    eng.close()
    return contigs, refs, recs, o, rp.jackknife_se(tot.fwd, fwd), rp.jackknife_se(tot.rev, rev)


def write_aln(path: Path, fmt: str, refs, recs):
    if fmt == "bam":
        tl.write_bam(path, refs, recs, rng=np.random.default_rng(2))
    else:
        tl.write_sam(path, refs, recs)


def check_printed(printed: str, want: float):
    """A value the file prints with "%.5e" against the numpy jackknife.  The two computations may differ by a relative
    2e-6; the six digits of the format then round the value by up to half a unit of its sixth digit (a relative 5e-6 at
    a mantissa of 1, more than the 2e-6 alone would allow), so that half unit is granted on top.  An exact 0 prints as 0."""
    if want == 0.0:
        assert printed == "0.00000e+00", printed
        return
    half_unit = 0.5 * 10.0 ** (int(printed.split("e")[1]) - 5)
    assert abs(float(printed) - want) <= 2e-6 * want + half_unit, (printed, want)


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_J(pkg, cli_case, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    contigs, refs, recs, o, se_f, se_r = cli_case
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, contigs)
    aln = tmp_path / f"in.{fmt}"
    write_aln(aln, fmt, refs, recs)
    env = {**os.environ, **extra}
    prefix = tmp_path / "out"

    def run(out, *more):
        return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(out), *more] + o.argv(), capture_output=True, text=True,
                              env=env, timeout=300)

    pr = run(prefix, "-J", str(CLI_K))
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(f" -J {CLI_K}")
    assert sorted(p.name for p in tmp_path.glob("out.*")) == ["out.pss.counts.txt", "out.pss.rates.se.txt", "out.pss.rates.txt"]
    # counts and rates: byte-identical to the same command without -J, which writes no standard-error file
    plain = tmp_path / "plain"
    pr = run(plain)
    assert pr.returncode == 0, pr.stderr
    for kind in ("counts", "rates"):
        assert Path(f"{plain}.pss.{kind}.txt").read_bytes().replace(b"plain.pss", b"out.pss") == Path(f"{prefix}.pss.{kind}.txt").read_bytes()
    assert sorted(p.name for p in tmp_path.glob("plain.*")) == ["plain.pss.counts.txt", "plain.pss.rates.txt"]
    head, ((lab_f, val_f), (lab_r, val_r)) = rp.parse_rates_text(Path(f"{prefix}.pss.rates.se.txt").read_text())
    rhead, _ = rp.parse_rates_text(Path(f"{prefix}.pss.rates.txt").read_text())
    assert head[3] == f"### OUT: {prefix}.pss.rates.se.txt" and head[:3] == rhead[:3] and head[4:10] == rhead[4:10]
    assert head[10:] == [f"### jackknife standard errors of the {w} read substitution rates, K = {CLI_K} read-name replicates"
                         for w in ("forward", "reverse")]
    n = o.region_len
    assert lab_f == list(range(n)) and lab_r == list(range(n - 1, -1, -1))
    nonzero = 0
    for pos in range(n):
        for c in range(12):
            check_printed(val_f[pos][c], float(se_f[pos, c]))
            check_printed(val_r[n - 1 - pos][c], float(se_r[pos, c]))
            nonzero += float(val_f[pos][c]) > 0
    assert nonzero > 100 and se_f.max() > 1e-4
    pr = run(tmp_path / "bad", "-J", str(CLI_K), "-G")
    assert pr.returncode == 1 and pr.stderr.startswith("-J (jackknife replicates) and -G") and "exclude each other" in pr.stderr
    assert not list(tmp_path.glob("bad.*"))


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_replicate_1_of_3_of_setA_is_the_golden(pkg, kernel):
    """tests/golden/rep1of3_setA.pss.counts.txt: the unmodified reference on setA.sam reduced to replicate 1 of 3"""
    import site_context_lib as sc
    contigs = sc.read_fasta(GOLD / "setA.fa")
    refs, recs = ml.read_sam(GOLD / "setA.sam")
    eng = run_engine(pkg, contigs, refs, recs, tl.PssOpts(), kern_of(pkg, kernel), replicates=3)
    fwd, rev = eng.finish_replicates()
    eng.close()
    wf, wr = tl.parse_counts_text((GOLD / "rep1of3_setA.pss.counts.txt").read_text())
    assert wf[2:].sum() > 0 and np.array_equal(fwd[1], wf) and np.array_equal(rev[1], wr)

"""fragkon -S / -G / -C on the GPU: one pair of k-mer tables (5' / 3' fragmentation-point contexts) per read-length
bin, per @RG ID or per contig set, in one pass over the records.  Every plane must equal what fragkon computes the
restricted way -- `-l <lo> -L <hi>`, the records `samtools view -r <ID>` keeps, a genome cut down to the set's
contigs -- as given by the CPU oracle (pinned to the reference by test_oracle_vs_ref.py), by the same binary run
that way and, when oracle/_ref exists, by the reference's own fragkon.  Every comparison is exact integer equality.

The length bins go by strlen(SEQ), the length fragkon's -l / -L compare for paired reads too, not by |TLEN| as
pss-bam's bins do: the fixture is checked to hold records that pass fragkon's filters and whose two lengths fall
into different bins."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

KS = [2, 3, 4, 5, 8]   # both sides of KMER_LDS_MAX_K (4), odd k
REJECT = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
DROP = ("slow_path",)


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def fk_dict(o: tl.FkOpts) -> dict:
    return dict(klen=o.klen, min_mq=o.min_mq, min_read_len=o.min_read_len, max_read_len=o.max_read_len, merged_only=o.merged_only)


def kern_of(pkg, name):
    return pkg.KERNEL_TILED if name == "TILED" else pkg.KERNEL_SIMPLE


def bins_of(o: tl.FkOpts, edges: list[int]) -> list[tuple[int, int]]:
    return list(zip([o.min_read_len] + edges, [e - 1 for e in edges] + [o.max_read_len]))


def random_edges(rng, o: tl.FkOpts, k: int) -> list[int]:
    """k rising edges inside (l, min(L, 270)]: the fuzz lengths run 1..260"""
    pool = np.arange(o.min_read_len + 1, min(o.max_read_len, 270) + 1)
    return sorted(int(x) for x in rng.choice(pool, size=min(k, len(pool)), replace=False))


def bin_index(edges, length):
    return sum(1 for e in edges if e <= length)


def parting_records(recs, contig_names, edges):
    """records fragkon tallies as one end of a pair (proper, mate mapped, read1 or read2, CIGAR <strlen(SEQ)>M on a
    contig of the genome) whose strlen(SEQ) and |TLEN| lie in different bins of `edges`"""
    out = []
    for r in recs:
        if not (r.flag & 0x1) or (r.flag & REJECT) or (r.flag & 0xA) != 0x2 or not (r.flag & 0xC0):
            continue
        if r.rname not in contig_names or r.pos < 10 or r.seq == "*" or r.qual == "*" or r.cigar != [(len(r.seq), "M")]:
            continue
        if bin_index(edges, len(r.seq)) != bin_index(edges, abs(r.tlen)):
            out.append(r)
    return out


def same_tables(a, k5, k3):
    return np.array_equal(a.k5, k5.astype(np.uint64)) and np.array_equal(a.k3, k3.astype(np.uint64))


def plane0(eng):
    k5 = np.ones(4 ** eng.klen, dtype=np.uint64)
    k3 = np.ones_like(k5)
    assert eng._L.pssbam_engine_finish_kmer_groups(eng._h, -1, k5.ctypes.data, k3.ctypes.data) == 0
    return k5, k3


def make_engine(pkg, contigs, refs, o: tl.FkOpts, kernel, **planes):
    eng = pkg.Engine(kmer=fk_dict(o), kernel=kernel, **planes)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    return eng


def check_totals(pkg, contigs, refs, raw, o, kernel, tot, oracle=None, g=None, sam=None):
    """the totals and the status counters of an engine with planes == those of the same engine without"""
    plain = make_engine(pkg, contigs, refs, o, kernel)
    plain.submit(raw)
    want = plain.finish()
    plain.close()
    assert np.array_equal(tot.k5, want.k5) and np.array_equal(tot.k3, want.k3)
    assert {k: v for k, v in tot.stats.items() if k not in DROP} == {k: v for k, v in want.stats.items() if k not in DROP}
    if oracle is not None:
        k5, k3, _ = oracle.fragkon(g, sam, o)
        assert same_tables(tot, k5, k3)


def check_bins(pkg, oracle, fz, o, edges, kernel):
    contigs, refs, recs, sam, g, raw = fz
    eng = make_engine(pkg, contigs, refs, o, kernel, length_bins=edges)
    eng.submit(raw)
    got = eng.finish_bins()
    assert list(got) == bins_of(o, edges)
    for lo, hi in bins_of(o, edges):
        k5, k3, _ = oracle.fragkon(g, sam, tl.FkOpts(**{**fk_dict(o), "min_read_len": lo, "max_read_len": hi}))
        assert same_tables(got[(lo, hi)], k5, k3), ((lo, hi), o, edges)
    tot = eng.finish()
    assert np.array_equal(sum(t.k5 for t in got.values()), tot.k5) and np.array_equal(sum(t.k3 for t in got.values()), tot.k3)
    p5, p3 = plane0(eng)
    assert not p5.any() and not p3.any()
    eng.close()
    check_totals(pkg, contigs, refs, raw, o, kernel, tot, oracle, g, sam)
    return got, tot


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(7301, 3000)
    sam = tmp_path_factory.mktemp("kplanes") / "all.sam"
    tl.write_sam(sam, refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    # the selector must read strlen(SEQ), not |TLEN|: only records whose two lengths part can tell
    assert len(parting_records(recs, {c[0] for c in contigs}, [30, 60])) >= 5
    yield contigs, refs, recs, sam, g, tl.raw_records(refs, recs)
    oracle.free_genome(g)


# ---- 1. engine vs oracle -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("k", KS)
def test_engine_kmer_bins_match_oracle(pkg, oracle, fuzz, kernel, k):
    rng = np.random.default_rng(500 + k)
    contigs, _, recs = fuzz[0], fuzz[1], fuzz[2]
    for n_edges in (1, 4, 9, 63):
        o = tl.random_fk_opts(rng)
        o.klen = k
        if n_edges == 63:
            o.min_read_len, o.max_read_len = 0, 250000000
        edges = list(range(8, 8 + 4 * 63, 4)) if n_edges == 63 else random_edges(rng, o, n_edges)
        got, tot = check_bins(pkg, oracle, fuzz, o, edges, kern_of(pkg, kernel))
        if n_edges == 63:
            assert tot.k5.sum() > 0 and tot.k3.sum() > 0
            assert parting_records(recs, {c[0] for c in contigs}, edges)
    # the fixed edges of the fixture's check, with filters that let the parting records through
    o = tl.FkOpts(klen=k)
    got, _ = check_bins(pkg, oracle, fuzz, o, [30, 60], kern_of(pkg, kernel))
    assert all(t.k5.sum() + t.k3.sum() > 0 for t in got.values())


@pytest.fixture(scope="module")
def fuzz_rg(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(7302, 3000, with_rg=True)
    d = tmp_path_factory.mktemp("kplanes_rg")
    sams = {}
    for gid in ("grpA", "grpB", None):
        if gid is None:
            keep = [r for r in recs if not any(t[0] == "RG" for t in r.tags)]
        else:
            keep = [r for r in recs if next((t for t in r.tags if t[0] == "RG"), None) == ("RG", "Z", gid)]
        sams[gid] = d / f"{gid}.sam"
        tl.write_sam(sams[gid], refs, keep)
    tl.write_sam(d / "all.sam", refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    yield contigs, refs, recs, d / "all.sam", g, tl.raw_records(refs, recs), sams
    oracle.free_genome(g)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("k", KS)
def test_engine_kmer_read_groups_match_oracle(pkg, oracle, fuzz_rg, kernel, k):
    contigs, refs, recs, sam, g, raw, sams = fuzz_rg
    rng = np.random.default_rng(600 + k)
    for o in (tl.FkOpts(klen=k), tl.random_fk_opts(rng)):
        o.klen = k
        eng = make_engine(pkg, contigs, refs, o, kern_of(pkg, kernel), read_groups=["grpA", "grpB", "absent"])
        eng.submit(raw)
        got = eng.finish_groups()
        assert list(got) == [None, "grpA", "grpB", "absent"]
        for gid in ("grpA", "grpB", None):
            k5, k3, _ = oracle.fragkon(g, sams[gid], o)
            assert same_tables(got[gid], k5, k3), (gid, o)
        assert not got["absent"].k5.any() and not got["absent"].k3.any()
        tot = eng.finish()
        assert np.array_equal(sum(t.k5 for t in got.values()), tot.k5) and np.array_equal(sum(t.k3 for t in got.values()), tot.k3)
        eng.close()
        check_totals(pkg, contigs, refs, raw, o, kern_of(pkg, kernel), tot, oracle, g, sam)
    assert got["grpA"].k5.sum() > 0 and got["grpB"].k3.sum() > 0 and got[None].k5.sum() > 0


SETS = {"big": ["chrB", "chrMissing"], "chrA": ["chrA"], "small": ["tiny.4", "nowhere"]}   # scaffold_10 stays in plane 0


def oracle_on_contigs(oracle, contigs, names, sam, o):
    keep = [c for c in contigs if c[0] in names]
    if not keep:
        return np.zeros(4 ** o.klen, dtype=np.uint32), np.zeros(4 ** o.klen, dtype=np.uint32)
    g = oracle.genome_from_arrays(tl.loaded_contigs(keep))
    try:
        k5, k3, _ = oracle.fragkon(g, sam, o)
    finally:
        oracle.free_genome(g)
    return k5, k3


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("k", KS)
def test_engine_kmer_contig_sets_match_oracle(pkg, oracle, tmp_path, kernel, k):
    contigs, refs, recs = tl.fuzz_dataset(7303, 3000, contig_lens=(5000, 1200, 300, 900))
    sam = tmp_path / "all.sam"
    tl.write_sam(sam, refs, recs)
    raw = tl.raw_records(refs, recs)
    rng = np.random.default_rng(700 + k)
    listed = {nm for nms in SETS.values() for nm in nms}
    for o in (tl.FkOpts(klen=k), tl.random_fk_opts(rng)):
        o.klen = k
        eng = make_engine(pkg, contigs, refs, o, kern_of(pkg, kernel), contig_sets=SETS)
        eng.submit(raw)
        got = eng.finish_sets()
        assert list(got) == list(SETS)
        for label, names in SETS.items():
            k5, k3 = oracle_on_contigs(oracle, contigs, names, sam, o)
            assert same_tables(got[label], k5, k3), (label, o)
        p5, p3 = plane0(eng)
        k5, k3 = oracle_on_contigs(oracle, contigs, {c[0] for c in contigs} - listed, sam, o)
        assert np.array_equal(p5, k5.astype(np.uint64)) and np.array_equal(p3, k3.astype(np.uint64))
        tot = eng.finish()
        assert np.array_equal(sum(t.k5 for t in got.values()) + p5, tot.k5)
        assert np.array_equal(sum(t.k3 for t in got.values()) + p3, tot.k3)
        eng.close()
        check_totals(pkg, contigs, refs, raw, o, kern_of(pkg, kernel), tot)
    assert got["big"].k5.sum() > 0 and got["chrA"].k5.sum() > 0 and got["small"].k3.sum() > 0 and p5.sum() > 0


# ---- 2. plane passes and the overflow path -------------------------------------------------------------------------

def test_engine_kmer_plane_passes(pkg, oracle, fuzz, monkeypatch):
    """PSSBAM_GROUP_SLOTS=2: five bins and plane 0 take three launches at k = 4; the deltas belong to the first"""
    monkeypatch.setenv("PSSBAM_GROUP_SLOTS", "2")
    check_bins(pkg, oracle, fuzz, tl.FkOpts(klen=4, min_mq=5), [30, 50, 70, 150], pkg.KERNEL_TILED)


@pytest.mark.parametrize("k", [4, 8])
def test_engine_kmer_overflow_path(pkg, oracle, fuzz, fuzz_rg, monkeypatch, k):
    """records longer than the staged prefix take the one-lane path; -G stages whole records"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    _, tot = check_bins(pkg, oracle, fuzz, tl.FkOpts(klen=k), [20, 45, 60, 90, 200], pkg.KERNEL_TILED)
    assert tot.stats["slow_path"] > 0
    contigs, refs, recs, sam, g, raw, sams = fuzz_rg
    o = tl.FkOpts(klen=k)
    eng = make_engine(pkg, contigs, refs, o, pkg.KERNEL_TILED, read_groups=["grpB", "grpA"])
    eng.submit(raw)
    got = eng.finish_groups()
    for gid in ("grpA", "grpB", None):
        k5, k3, _ = oracle.fragkon(g, sams[gid], o)
        assert same_tables(got[gid], k5, k3), gid
    assert eng.finish().stats["slow_path"] > 0
    eng.close()


# ---- 3. feed, reset, accumulation, two engines ---------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 8])
def test_submit_bgzf_kmer_bins_set_after_feed_open(pkg, oracle, tmp_path, k):
    contigs, refs, recs = tl.fuzz_dataset(7304, 4000)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    sam = tmp_path / "all.sam"
    tl.write_sam(sam, refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        o = tl.FkOpts(klen=k, min_mq=5)
        edges = [35, 50, 80, 120]
        eng = pkg.Engine(kmer=fk_dict(o))
        eng.feed_open(len(refs))
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        eng.set_length_bins(edges)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        got = eng.finish_bins()
        for lo, hi in bins_of(o, edges):
            k5, k3, _ = oracle.fragkon(g, sam, tl.FkOpts(**{**fk_dict(o), "min_read_len": lo, "max_read_len": hi}))
            assert same_tables(got[(lo, hi)], k5, k3), (lo, hi)
        assert eng.feed_status()["flags"] == 0
        assert eng.finish().stats["records"] == len(recs)
        eng.close()
    finally:
        oracle.free_genome(g)


@pytest.mark.parametrize("k", [3, 8])
def test_kmer_planes_reset_accumulate_and_sum_of_two_engines(pkg, fuzz, k):
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")                     # reads a counter block back, straight from the HIP runtime
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    contigs, refs, recs, sam, g, raw = fuzz
    o = tl.FkOpts(klen=k)
    edges = [25, 40, 64, 100]
    eng = make_engine(pkg, contigs, refs, o, pkg.KERNEL_TILED, length_bins=edges)
    eng.submit(raw)
    once = eng.finish_bins()
    eng.reset()                                             # the bins survive reset
    assert eng.length_bins == bins_of(o, edges)
    half = len(recs) // 2
    raw_a, raw_b = tl.raw_records(refs, recs[:half]), tl.raw_records(refs, recs[half:])
    eng.submit(raw_a)
    eng.submit(raw_b)                                       # accumulation over two submits
    twice = eng.finish_bins()
    assert all(np.array_equal(once[b].k5, twice[b].k5) and np.array_equal(once[b].k3, twice[b].k3) for b in once)
    lay = eng.counter_layout()
    d, n = eng.counters_device()
    assert lay["n_u64"] == n
    nb = 4 ** k
    assert lay["length_bins"][1]["k5"] == lay["stats"] + pkg.ST_N + 2 * nb and lay["length_bins"][1]["k3"] == lay["length_bins"][1]["k5"] + nb

    def block(e):
        e.sync()
        ptr, n_u64 = e.counters_device()
        out = np.zeros(n_u64, dtype=np.uint64)
        assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
        return out

    whole = block(eng)
    parts = []
    for part in (raw_a, raw_b):                             # two engines, half of the records each
        e2 = make_engine(pkg, contigs, refs, o, pkg.KERNEL_TILED, length_bins=edges)
        e2.submit(part)
        parts.append(block(e2))
        e2.close()
    assert np.array_equal(parts[0] + parts[1], whole)       # the blocks add as plain u64 arrays
    for i, b in enumerate(bins_of(o, edges)):
        at = lay["length_bins"][i]
        assert np.array_equal(whole[at["k5"]:at["k5"] + nb], once[b].k5) and np.array_equal(whole[at["k3"]:at["k3"] + nb], once[b].k3)
    eng.close()


# ---- 4. rules ------------------------------------------------------------------------------------------------------

def test_kmer_planes_rules(pkg):
    E = pkg.PssbamError
    EINVAL = -1
    for sel in (dict(length_bins=[30]), dict(read_groups=["a"]), dict(contig_sets={"x": ["chrA"]})):
        with pytest.raises(E):                              # pss + k-mer together: no planes
            pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), **sel)
    eng = pkg.Engine(kmer=dict(klen=4), length_bins=[30])
    one = np.zeros(6 * 16 * 2, dtype=np.uint64)
    assert eng._L.pssbam_engine_finish_groups(eng._h, 0, one.ctypes.data, one.ctypes.data) == EINVAL
    with pytest.raises(E):                                  # one selector at a time
        eng.set_read_groups(["a"])
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), length_bins=[30])
    k = np.zeros(4 ** 4, dtype=np.uint64)
    assert eng._L.pssbam_engine_finish_kmer_groups(eng._h, 0, k.ctypes.data, k.ctypes.data) == EINVAL
    eng.close()
    eng = pkg.Engine(kmer=dict(klen=5, min_read_len=20, max_read_len=80))
    for bad in ([], [20], [30, 30], [40, 30], [81], list(range(21, 85))):
        with pytest.raises(E, match=r"pssbam error -1:"):   # PSSBAM_EINVAL
            eng.set_length_bins(bad)
    eng.set_length_bins([21, 80])                           # l + 1 and L themselves
    assert eng.length_bins == [(20, 20), (21, 79), (80, 80)]
    eng.close()
    eng = pkg.Engine(kmer=dict(klen=3), read_group="grpA", contig_sets={"x": ["chrA"]})   # allowed with -R
    assert eng.counter_layout()["n_u64"] == eng.counters_device()[1]
    eng.close()


# ---- 5. the command line -------------------------------------------------------------------------------------------

CLI_MODES = {
    "bam_device_feed": ("bam", {}),
    "bam_host_reader": ("bam", {"PSSBAM_DEVICE_INFLATE": "0"}),
    "sam": ("sam", {}),
    "bam_two_gpus": ("bam", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}),
}


def write_aln(path: Path, fmt, refs, recs, text_header=None):
    if fmt == "bam" and text_header is None:
        tl.write_bam(path, refs, recs, rng=np.random.default_rng(2))
    elif fmt == "bam":
        raw = tl.bam_bytes(refs, recs, text_header)
        with open(path, "wb") as fh:
            for i in range(0, len(raw), 0xE000):
                fh.write(tl.bgzf_block(raw[i:i + 0xE000], 1))
            fh.write(tl.BGZF_EOF)
    elif text_header is not None:
        path.write_text(text_header + "".join(tl.sam_line(r) for r in recs))
    else:
        tl.write_sam(path, refs, recs)


def run_fragkon(exe, fa, aln, o, env, cwd, extra=()):
    pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln)] + o.argv() + list(extra), capture_output=True, text=True,
                        env=env, timeout=300, cwd=cwd)
    assert pr.returncode == 0, pr.stderr
    return pr.stdout


def table_of(text: str) -> str:
    """from the `# KMER` line on: the `###` lines in front echo the file names given"""
    return text[text.index("# KMER"):]


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_S_matches_l_L_per_bin(pkg, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "fragkon"
    o = tl.FkOpts(klen=4, min_mq=10, min_read_len=10)
    contigs, refs, recs = tl.fuzz_dataset(7305, 6000)
    recs = tl.ref_safe(recs, o.klen)
    assert parting_records(recs, {c[0] for c in contigs}, [25, 40, 64])
    tl.write_fasta(tmp_path / "g.fa", contigs)
    write_aln(tmp_path / f"in.{fmt}", fmt, refs, recs)
    env = {**os.environ, **extra}
    fa, aln = "g.fa", f"in.{fmt}"
    plain = run_fragkon(exe, fa, aln, o, env, tmp_path)
    assert run_fragkon(exe, fa, aln, o, env, tmp_path, ["-S", "25,40,64", "-o", "out"]) == plain
    assert len(list(tmp_path.glob("out.*.fragkon.txt"))) == 4
    use_ref = tl.have_ref() and mode in ("bam_device_feed", "sam")
    s5 = s3 = 0
    for lo, hi in bins_of(o, [25, 40, 64]):
        got = (tmp_path / f"out.len{lo}-{hi}.fragkon.txt").read_text()
        ob = tl.FkOpts(**{**fk_dict(o), "min_read_len": lo, "max_read_len": hi})
        assert run_fragkon(exe, fa, aln, ob, env, tmp_path) == got, (lo, hi)
        if use_ref:
            _, _, want, _ = tl.run_ref_fragkon(tmp_path / fa, tmp_path / aln, ob, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
            assert table_of(want) == table_of(got), (lo, hi)
        k5, k3 = tl.parse_fragkon_text(got)
        s5, s3 = s5 + k5.astype(np.uint64), s3 + k3.astype(np.uint64)
    t5, t3 = tl.parse_fragkon_text(plain)
    assert np.array_equal(s5, t5) and np.array_equal(s3, t3) and t5.sum() > 0


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_G_matches_filtered_input_per_group(pkg, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "fragkon"
    o = tl.FkOpts(klen=5, min_mq=5)
    contigs, refs, recs = tl.fuzz_dataset(7306, 5000, with_rg=True)
    recs = tl.ref_safe(recs, o.klen)
    hdr = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs) + "@RG\tID:grpA\tSM:a\n@RG\tID:grpB\tSM:b\n"
    tl.write_fasta(tmp_path / "g.fa", contigs)
    write_aln(tmp_path / f"in.{fmt}", fmt, refs, recs, hdr)
    env = {**os.environ, **extra}
    plain = run_fragkon(exe, "g.fa", f"in.{fmt}", o, env, tmp_path)
    assert run_fragkon(exe, "g.fa", f"in.{fmt}", o, env, tmp_path, ["-G", "-o", "out"]) == plain
    assert sorted(p.name for p in tmp_path.glob("out.*.fragkon.txt")) == ["out.grpA.fragkon.txt", "out.grpB.fragkon.txt"]
    use_ref = tl.have_ref() and mode in ("bam_device_feed", "sam")
    for gid in ("grpA", "grpB"):
        keep = [r for r in recs if next((t for t in r.tags if t[0] == "RG"), None) == ("RG", "Z", gid)]
        write_aln(tmp_path / f"{gid}.{fmt}", fmt, refs, keep, hdr)
        got = (tmp_path / f"out.{gid}.fragkon.txt").read_text()
        assert table_of(run_fragkon(exe, "g.fa", f"{gid}.{fmt}", o, env, tmp_path)) == table_of(got), gid
        if use_ref:
            _, _, want, _ = tl.run_ref_fragkon(tmp_path / "g.fa", tmp_path / f"{gid}.{fmt}", o, bam2sam=str(exe.parent / "bam2sam"),
                                               timeout=300)
            assert table_of(want) == table_of(got), gid
        assert sum(tl.parse_fragkon_text(got)[0]) > 0


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_C_matches_reduced_fasta_per_set(pkg, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "fragkon"
    o = tl.FkOpts(klen=3, min_mq=5)
    contigs, refs, recs = tl.fuzz_dataset(7307, 5000, contig_lens=(5000, 1200, 300, 900))
    recs = tl.ref_safe(recs, o.klen)
    tl.write_fasta(tmp_path / "g.fa", contigs)
    write_aln(tmp_path / f"in.{fmt}", fmt, refs, recs)
    (tmp_path / "map.tsv").write_text("".join(f"{nm}\t{label}\n" for label, nms in SETS.items() for nm in nms))
    env = {**os.environ, **extra}
    plain = run_fragkon(exe, "g.fa", f"in.{fmt}", o, env, tmp_path)
    assert run_fragkon(exe, "g.fa", f"in.{fmt}", o, env, tmp_path, ["-C", "map.tsv", "-o", "out"]) == plain
    assert len(list(tmp_path.glob("out.*.fragkon.txt"))) == len(SETS)
    use_ref = tl.have_ref() and mode in ("bam_device_feed", "sam")
    for label, names in SETS.items():
        sub = tmp_path / f"only_{label}"
        sub.mkdir()
        tl.write_fasta(sub / "g.fa", [c for c in contigs if c[0] in names])   # the same relative -F name
        os.symlink(tmp_path / f"in.{fmt}", sub / f"in.{fmt}")
        got = (tmp_path / f"out.{label}.fragkon.txt").read_text()
        assert run_fragkon(exe, "g.fa", f"in.{fmt}", o, env, sub) == got, label
        if use_ref:
            _, _, want, _ = tl.run_ref_fragkon(sub / "g.fa", sub / f"in.{fmt}", o, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
            assert table_of(want) == table_of(got), label
        assert sum(tl.parse_fragkon_text(got)[0]) > 0

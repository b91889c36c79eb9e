"""pss-bam -S on the GPU: one set of substitution tables per fragment-length bin in one pass over the records.
Every bin's tables must equal what `-l <lo> -L <hi>` gives (the CPU oracle; for the command line also the same
binary run with -l / -L, and the reference itself when oracle/_ref exists), the bins must sum to the totals,
and the totals must equal an unbinned run."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq,
                up_ctx=o.up_ctx, down_ctx=o.down_ctx, merged_only=o.merged_only)


def bins_of(o: tl.PssOpts, edges: list[int]) -> list[tuple[int, int]]:
    return list(zip([o.min_read_len] + edges, [e - 1 for e in edges] + [o.max_read_len]))


def random_edges(rng, o: tl.PssOpts, k: int) -> list[int]:
    """k rising edges inside (l, min(L, 270)]: the fuzz lengths run 1..260, so the last bin may be empty"""
    top = min(o.max_read_len, 270)
    pool = np.arange(o.min_read_len + 1, top + 1)
    return sorted(int(x) for x in rng.choice(pool, size=min(k, len(pool)), replace=False))


def oracle_bins(oracle, g, sam: Path, o: tl.PssOpts, edges: list[int]) -> dict:
    out = {}
    for lo, hi in bins_of(o, edges):
        f, r, _ = oracle.pss(g, sam, tl.PssOpts(**{**pss_dict(o), "min_read_len": lo, "max_read_len": hi,
                                                   "read_group": o.read_group}))
        out[(lo, hi)] = (f, r)
    return out


def plane0(eng):
    fwd = np.ones((eng.region_len + 2, 16), dtype=np.uint64)
    rev = np.ones_like(fwd)
    assert eng._L.pssbam_engine_finish_groups(eng._h, -1, fwd.ctypes.data, rev.ctypes.data) == 0
    return fwd, rev


def run_engine(pkg, contigs, refs, raw, o: tl.PssOpts, kernel, edges=None):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_group=o.read_group, length_bins=edges)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(raw)
    return eng


def check_bins(pkg, oracle, contigs, refs, recs, sam, g, o, edges, kernel):
    """bins == oracle per -l/-L window, bins sum to the totals, totals == unbinned run, plane 0 empty"""
    raw = tl.raw_records(refs, recs)
    want = oracle_bins(oracle, g, sam, o, edges)
    eng = run_engine(pkg, contigs, refs, raw, o, kernel, edges)
    got = eng.finish_bins()
    assert list(got) == bins_of(o, edges)
    for key, (wf, wr) in want.items():
        assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), (key, o, edges)
    tot = eng.finish()
    assert np.array_equal(sum(t.fwd for t in got.values()), tot.fwd)
    assert np.array_equal(sum(t.rev for t in got.values()), tot.rev)
    p0f, p0r = plane0(eng)
    assert not p0f.any() and not p0r.any()
    eng.close()
    plain = run_engine(pkg, contigs, refs, raw, o, kernel)
    ref_tot = plain.finish()
    plain.close()
    assert np.array_equal(tot.fwd, ref_tot.fwd) and np.array_equal(tot.rev, ref_tot.rev)
    drop = ("slow_path",)
    assert {k: v for k, v in tot.stats.items() if k not in drop} == {k: v for k, v in ref_tot.stats.items() if k not in drop}
    return tot


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(7101, 3000)
    sam = tmp_path_factory.mktemp("lenbins") / "all.sam"
    tl.write_sam(sam, refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    yield contigs, refs, recs, sam, g
    oracle.free_genome(g)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("n", [15, 25, 31, 62])
def test_engine_bins_match_oracle(pkg, oracle, fuzz, kernel, n):
    contigs, refs, recs, sam, g = fuzz
    rng = np.random.default_rng(100 + n)
    kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
    for k in (1, 4, 9):
        o = tl.random_pss_opts(rng)
        o.region_len = n
        check_bins(pkg, oracle, contigs, refs, recs, sam, g, o, random_edges(rng, o, k), kern)


def test_engine_bins_overflow_path(pkg, oracle, fuzz, monkeypatch):
    """records longer than the staged prefix take the one-lane length-bin path"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    contigs, refs, recs, sam, g = fuzz
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        tot = check_bins(pkg, oracle, contigs, refs, recs, sam, g, o, [20, 45, 60, 90, 200], pkg.KERNEL_TILED)
        assert tot.stats["slow_path"] > 0


@pytest.mark.parametrize("n", [15, 40])
def test_engine_bins_plane_passes(pkg, oracle, fuzz, monkeypatch, n):
    """63 edges (65 planes) do not fit one launch's LDS; PSSBAM_GROUP_SLOTS=2 forces passes with a few bins"""
    contigs, refs, recs, sam, g = fuzz
    o = tl.PssOpts(region_len=n, min_mq=5)
    check_bins(pkg, oracle, contigs, refs, recs, sam, g, o, list(range(10, 10 + 4 * 63, 4)), pkg.KERNEL_TILED)
    monkeypatch.setenv("PSSBAM_GROUP_SLOTS", "2")
    check_bins(pkg, oracle, contigs, refs, recs, sam, g, o, [30, 50, 70, 150], pkg.KERNEL_TILED)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_engine_bins_of_one_read_group(pkg, oracle, kernel, tmp_path, monkeypatch):
    """-S with -R: bins of the records -R keeps (whole records staged; short tiles push some onto the overflow path)"""
    if kernel == "TILED":
        monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    contigs, refs, recs = tl.fuzz_dataset(7102, 3000, with_rg=True)
    keep = [r for r in recs if ("RG", "Z", "grpA") in r.tags]
    sam = tmp_path / "keep.sam"
    tl.write_sam(sam, refs, keep)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        o = tl.PssOpts(region_len=25)
        edges = [30, 60, 100]
        want = oracle_bins(oracle, g, sam, o, edges)
        kern = pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE
        o_rg = tl.PssOpts(**{**pss_dict(o), "read_group": "grpA"})
        eng = run_engine(pkg, contigs, refs, tl.raw_records(refs, recs), o_rg, kern, edges)
        got = eng.finish_bins()
        for key, (wf, wr) in want.items():
            assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), key
        tot = eng.finish()
        assert tot.stats["rg_dropped"] == len(recs) - len(keep)
        eng.close()
    finally:
        oracle.free_genome(g)


def test_engine_bins_rules(pkg):
    E = pkg.PssbamError
    with pytest.raises(E):                                  # k-mer tables are not split
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), length_bins=[30])
    with pytest.raises(E):                                  # read groups set
        pkg.Engine(pss=dict(region_len=5), read_groups=["a"], length_bins=[30])
    eng = pkg.Engine(pss=dict(region_len=5), length_bins=[30])
    with pytest.raises(E):                                  # and the other way round
        eng.set_read_groups(["a"])
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=5, min_read_len=20, max_read_len=80))
    for bad in ([], [20], [30, 30], [40, 30], [81], list(range(21, 85))):
        with pytest.raises(E):
            eng.set_length_bins(bad)
    assert eng.length_bins == []
    eng.set_length_bins([21, 80])                           # l + 1 and L themselves
    assert eng.length_bins == [(20, 20), (21, 79), (80, 80)]
    eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), read_group="grpA", length_bins=[30, 60])   # allowed with -R
    lay = eng.counter_layout()
    assert [x["bin"] for x in lay["length_bins"]] == [(0, 29), (30, 59), (60, 250000000)]
    assert lay["n_u64"] == eng.counters_device()[1]
    assert lay["length_bins"][1]["fwd"] == lay["stats"] + pkg.ST_N + 2 * lay["rows"] * 16
    contigs, refs, recs = tl.fuzz_dataset(5, 300, with_rg=True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    with pytest.raises(E):                                  # records have been tallied
        eng.set_length_bins([40])
    first = eng.finish_bins()
    eng.reset()                                             # the bins survive reset
    assert eng.length_bins == [(0, 29), (30, 59), (60, 250000000)]
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_bins()
    assert all(np.array_equal(first[k].fwd, again[k].fwd) and np.array_equal(first[k].rev, again[k].rev) for k in first)
    eng.reset()
    eng.set_length_bins([40])                               # legal again after reset
    assert eng.length_bins == [(0, 39), (40, 250000000)]
    eng.close()
    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_length_bins([30])
    eng.close()
    other.close()


def test_submit_bgzf_bins_set_after_feed_open(pkg, oracle, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(7103, 4000)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    sam = tmp_path / "all.sam"
    tl.write_sam(sam, refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        o = tl.PssOpts(region_len=15, min_mq=5)
        edges = [35, 50, 80, 120]
        want = oracle_bins(oracle, g, sam, o, edges)
        eng = pkg.Engine(pss=pss_dict(o))
        eng.feed_open(len(refs))
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        eng.set_length_bins(edges)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        got = eng.finish_bins()
        for key, (wf, wr) in want.items():
            assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), key
        assert eng.feed_status()["flags"] == 0
        assert eng.finish().stats["records"] == len(recs)
        eng.close()
    finally:
        oracle.free_genome(g)


# ---- the command line ----------------------------------------------------------------------------------------------

CLI_MODES = {
    "bam_device_feed": ("bam", {}),
    "bam_host_reader": ("bam", {"PSSBAM_DEVICE_INFLATE": "0"}),
    "sam": ("sam", {}),
    "bam_two_gpus": ("bam", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}),
}


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_S_matches_l_L_per_bin(pkg, oracle, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    contigs, refs, recs = tl.fuzz_dataset(7104, 6000)
    recs = tl.ref_safe(recs)
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, contigs)
    aln = tmp_path / f"in.{fmt}"
    if fmt == "bam":
        tl.write_bam(aln, refs, recs, rng=np.random.default_rng(2))
    else:
        tl.write_sam(aln, refs, recs)
    o = tl.PssOpts(region_len=25, min_mq=10, min_read_len=10)
    edges_arg = "25,40,64,100"                      # a bin below -r is written too, empty: 10-24
    edges = [int(x) for x in edges_arg.split(",")]
    env = {**os.environ, **extra}
    prefix = tmp_path / "out"
    pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), "-S", edges_arg] + o.argv(),
                        capture_output=True, text=True, env=env, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(f" -S {edges_arg}")
    tot_c, tot_r = Path(f"{prefix}.pss.counts.txt").read_text(), Path(f"{prefix}.pss.rates.txt").read_text()
    files = {}
    for lo, hi in bins_of(o, edges):
        tagged = f"{prefix}.len{lo}-{hi}"
        files[(lo, hi)] = (Path(f"{tagged}.pss.counts.txt").read_text(), Path(f"{tagged}.pss.rates.txt").read_text(), tagged)
    assert len(list(tmp_path.glob("out.*.txt"))) == 2 * (len(edges) + 2)
    # the totals: byte-identical to the same command without -S
    pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix)] + o.argv(), capture_output=True, text=True,
                        env=env, timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert Path(f"{prefix}.pss.counts.txt").read_text() == tot_c
    assert Path(f"{prefix}.pss.rates.txt").read_text() == tot_r
    # every bin: byte-identical to -l <lo> -L <hi> -o <prefix>.len<lo>-<hi> (this binary, and the reference when present)
    use_ref = tl.have_ref() and mode in ("bam_device_feed", "sam")
    sum_f = sum_r = 0
    for (lo, hi), (ct, rt, tagged) in files.items():
        ob = tl.PssOpts(**{**pss_dict(o), "min_read_len": lo, "max_read_len": hi})
        pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", tagged] + ob.argv(), capture_output=True, text=True,
                            env=env, timeout=300)
        assert pr.returncode == 0, pr.stderr
        assert Path(f"{tagged}.pss.counts.txt").read_text() == ct, (lo, hi)
        assert Path(f"{tagged}.pss.rates.txt").read_text() == rt, (lo, hi)
        if use_ref:
            _, _, wc, wr, _ = tl.run_ref_pss(fa, aln, Path(tagged), ob, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
            assert wc == ct and wr == rt, (lo, hi)
        f, r = tl.parse_counts_text(ct)
        sum_f, sum_r = sum_f + f, sum_r + r
        if hi < o.region_len:
            assert not f.any() and not r.any()
    tf, trv = tl.parse_counts_text(tot_c)
    assert np.array_equal(tf, sum_f) and np.array_equal(trv, sum_r)

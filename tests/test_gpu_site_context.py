"""pss-bam -X cpg on the GPU: a second pair of tables, IN, over the interior positions whose reference site is in CpG
context, from the same pass as the ordinary tables T.

The specification is site_context_lib's: IN == the tool without -X on the same records with the read bases at every
other site set to N, and T - IN (rows 2+) == the same with the complementary mask.  So every check here runs the engine
(or the command) with the setting on the ORIGINAL records and compares with the CPU oracle (or the reference itself
when oracle/_ref exists) without it on the masked copies (checked on their own in test_site_context_host.py)."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import base_quality_lib as bq
import pssbam_testlib as tl
import regions_lib as rl
import site_context_lib as sc
from test_gpu_length_hist import CLI_MODES, pss_dict, write_aln

pytestmark = pytest.mark.gpu
SEED = 9401      # test_site_context_host.py checks on the CPU that this fixture is rich in both kinds of site


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def kern_of(pkg, kernel):
    return pkg.KERNEL_TILED if kernel == "TILED" else pkg.KERNEL_SIMPLE


def run_engine(pkg, contigs, refs, recs, o: tl.PssOpts, kernel, site="cpg", **kw):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_group=o.read_group, site_context=site, **kw)
    assert eng.site_context == site
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    if len(recs):
        eng.submit(tl.raw_records(refs, recs))
    return eng


def tables_of(pkg, contigs, refs, recs, o, kernel, **kw):
    """(T, (fwd_in, rev_in)) of one engine with the setting"""
    eng = run_engine(pkg, contigs, refs, recs, o, kernel, **kw)
    fin = eng.finish_site_context()
    tot = eng.finish()
    eng.close()
    return tot, fin


def stats_but(st: dict) -> dict:
    return {k: v for k, v in st.items() if k != "slow_path"}


def check_split(tot, fin, want_in, want_out, ctx=""):
    """IN == oracle on the keep-in mask, T - IN == oracle on the keep-out mask on rows 2+, rows 0/1 of IN are T's"""
    for t, got, w_in, w_out in ((tot.fwd, fin[0], want_in[0], want_out[0]), (tot.rev, fin[1], want_in[1], want_out[1])):
        assert np.array_equal(got, w_in), ctx
        assert np.array_equal(t[2:] - got[2:], w_out[2:]), ctx
        assert np.array_equal(got[:2], t[:2]) and np.array_equal(t[:2], w_out[:2]), ctx


@pytest.fixture(scope="module")
def fuzz(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(SEED, 3000)
    d = tmp_path_factory.mktemp("site")
    sams = {True: d / "in.sam", False: d / "out.sam"}
    for keep in (True, False):
        tl.write_sam(sams[keep], refs, sc.mask_recs(contigs, recs, keep))
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    yield contigs, refs, recs, sams, g
    oracle.free_genome(g)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("n", [15, 25, 31, 40, 62])
def test_engine_matches_oracle_on_masked_sams(pkg, oracle, fuzz, kernel, n):
    """one, two and three row passes; a count in the wrong pass or a missing neighbour at rows 31|32 or 61|62 shows here"""
    contigs, refs, recs, sams, g = fuzz
    rng = np.random.default_rng(500 + n)
    kern = kern_of(pkg, kernel)
    for trial in range(3):
        o = tl.random_pss_opts(rng) if trial else tl.PssOpts()
        o.region_len = n
        want_in, want_out = oracle.pss(g, sams[True], o)[:2], oracle.pss(g, sams[False], o)[:2]
        tot, fin = tables_of(pkg, contigs, refs, recs, o, kern)
        check_split(tot, fin, want_in, want_out, (kernel, n, o))
        eng = run_engine(pkg, contigs, refs, recs, o, kern, site=None)
        plain = eng.finish()
        eng.close()
        assert np.array_equal(tot.fwd, plain.fwd) and np.array_equal(tot.rev, plain.rev), (kernel, n, o)
        assert stats_but(tot.stats) == stats_but(plain.stats), (kernel, n, o)
        if not trial:
            assert fin[0][2:].sum() > 500 and (tot.fwd[2:] - fin[0][2:]).sum() > 500


# ---- one CG in a contig of A and T: every expected cell is known by hand ---------------------------------------------

SWEEP_L = 50


def sweep_case(n: int):
    """Forward- and reverse-strand reads of length SWEEP_L that copy the reference, placed so that the C of the one CG
    falls at every offset -2 .. n+1 from the left end and from the right end.  Expected IN: with the C at interior
    position i of an end (0 <= i < n) that end adds CC at row 2 + i, and the G -- one base further into the read seen
    from the left end, one base nearer the end seen from the right -- adds GG at its own row; a forward read's left end
    goes to the forward table and its right end to the reverse table, a reverse-strand read's ends go the other way
    round with both bases complemented (CC <-> GG)."""
    rng = np.random.default_rng(77)
    c = 300
    ctg = "".join("AT"[int(x)] for x in rng.integers(0, 2, size=c)) + "CG" + "".join("AT"[int(x)] for x in rng.integers(0, 2, size=c))
    recs = []
    fwd_in, rev_in = np.zeros((n + 2, 16), dtype=np.uint64), np.zeros((n + 2, 16), dtype=np.uint64)
    CC, GG = 5, 10
    for is_rev in (False, True):
        for d in range(-2, n + 2):
            for from_left in (True, False):
                s = c - d if from_left else c - (SWEEP_L - 1) + d
                recs.append(tl.Rec(f"s{len(recs):04d}", 16 if is_rev else 0, "one_cg", s + 1, 30, [(SWEEP_L, "M")],
                                   seq=ctg[s:s + SWEEP_L], qual="I" * SWEEP_L))
                for left_end in (True, False):
                    tab = (fwd_in if left_end else rev_in) if not is_rev else (rev_in if left_end else fwd_in)
                    for p, cell in ((c, CC), (c + 1, GG)):      # the two in-context positions of the contig
                        i = p - s if left_end else s + SWEEP_L - 1 - p
                        if 0 <= i < n:
                            tab[2 + i, 15 - cell if is_rev else cell] += 1
    return [("one_cg", ctg)], [("one_cg", len(ctg))], recs, (fwd_in, rev_in)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
@pytest.mark.parametrize("n", [30, 40])
def test_swept_dinucleotide(pkg, kernel, n):
    """pins the base beyond the window (the C one base in front of a window that starts with the G, the G one base
    behind a window that ends with the C) and the context-row neighbour (offsets -2, -1, n, n+1: nothing from the
    context rows, but the G at position 0 next to a C in the context row still counts)"""
    contigs, refs, recs, want = sweep_case(n)
    tot, fin = tables_of(pkg, contigs, refs, recs, tl.PssOpts(region_len=n), kern_of(pkg, kernel))
    assert tot.stats["pss_ok"] == len(recs) == 4 * (n + 4)
    for got, w, t in ((fin[0], want[0], tot.fwd), (fin[1], want[1], tot.rev)):
        assert np.array_equal(got[2:], w[2:]), (kernel, n, np.argwhere(got[2:] != w[2:])[:8])
        assert np.array_equal(got[:2], t[:2])
    assert fin[0][2:].sum() == fin[1][2:].sum() and fin[0][2:].sum() > 4 * (n - 2)


# ---- repeats ------------------------------------------------------------------------------------------------------------

def repeat_case(unit: str, n_reads=20000, L=40):
    ctg = unit * 1000
    rng = np.random.default_rng(11)
    starts = rng.integers(2, len(ctg) - L - 2, size=n_reads)
    recs = [tl.Rec(f"p{i:06d}", 16 * (i & 1), "rep", int(s) + 1, 30, [(L, "M")], seq=ctg[int(s):int(s) + L], qual="I" * L)
            for i, s in enumerate(starts)]
    return [("rep", ctg)], [("rep", len(ctg))], recs


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_repeats(pkg, kernel):
    kern = kern_of(pkg, kernel)
    o = tl.PssOpts(region_len=25)
    tot, fin = tables_of(pkg, *repeat_case("ACGT"), o, kern)          # every C is followed by a G
    assert tot.stats["pss_ok"] == 20000
    for got, t in ((fin[0], tot.fwd), (fin[1], tot.rev)):
        assert np.array_equal(got[2:, [5, 10]], t[2:, [5, 10]]) and t[2:, 5].min() > 1000
        rest = got[2:].copy()
        rest[:, [5, 10]] = 0
        assert not rest.any() and t[2:, [0, 15]].min() > 1000
    tot, fin = tables_of(pkg, *repeat_case("AGCT"), o, kern)          # GC, never CG
    assert tot.fwd[2:, 5].min() > 1000 and not fin[0][2:].any() and not fin[1][2:].any()


# ---- the one-lane path, other filters --------------------------------------------------------------------------------

def test_overflow_path(pkg, oracle, fuzz, monkeypatch):
    """records longer than the staged prefix take the one-lane path and give the same tables"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    contigs, refs, recs, sams, g = fuzz
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        tot, fin = tables_of(pkg, contigs, refs, recs, o, pkg.KERNEL_TILED)
        assert tot.stats["slow_path"] > 0
        check_split(tot, fin, oracle.pss(g, sams[True], o)[:2], oracle.pss(g, sams[False], o)[:2], n)


def masked_oracle(oracle, tmp_path, contigs, refs, recs, o, tag=""):
    """(oracle tables on the keep-in mask, on the keep-out mask) of `recs`"""
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        out = []
        for keep in (True, False):
            sam = tmp_path / f"m{tag}{int(keep)}.sam"
            tl.write_sam(sam, refs, sc.mask_recs(contigs, recs, keep))
            out.append(oracle.pss(g, sam, o)[:2])
        return out
    finally:
        oracle.free_genome(g)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_read_group_filter(pkg, oracle, kernel, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(9402, 3000, with_rg=True)
    keep = [r for r in recs if ("RG", "Z", "grpA") in r.tags]
    for n in (15, 40):
        o = tl.PssOpts(region_len=n, min_mq=3)
        want_in, want_out = masked_oracle(oracle, tmp_path, contigs, refs, keep, o, f"rg{n}")
        tot, fin = tables_of(pkg, contigs, refs, recs, tl.PssOpts(**{**pss_dict(o), "read_group": "grpA"}), kern_of(pkg, kernel))
        assert tot.stats["rg_dropped"] == len(recs) - len(keep) and fin[0][2:].sum() > 100
        check_split(tot, fin, want_in, want_out, (kernel, n))


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_min_base_quality(pkg, oracle, fuzz, kernel, tmp_path):
    """the two masks compose: a base masked by -Q is missing from T and from IN alike"""
    contigs, refs, recs, sams, g = fuzz
    low = bq.mask_recs(recs, 20)
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        want_in, want_out = masked_oracle(oracle, tmp_path, contigs, refs, low, o, f"q{n}")
        tot, fin = tables_of(pkg, contigs, refs, recs, o, kern_of(pkg, kernel), min_base_qual=20)
        check_split(tot, fin, want_in, want_out, (kernel, n))
        plain_in = oracle.pss(g, sams[True], o)[0]
        assert (fin[0][2:] != plain_in[2:]).any() and fin[0][2:].sum() > 100      # -Q did mask in-context bases


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_with_regions(pkg, oracle, kernel, tmp_path):
    contigs, refs, recs, ivs = rl.fuzz_case(rl.PSS_SEEDS[0])
    kept = rl.reduce_recs(recs, ivs)
    for n in (15, 40):
        o = tl.PssOpts(region_len=n)
        want_in, want_out = masked_oracle(oracle, tmp_path, contigs, refs, kept, o, f"t{n}")
        eng = run_engine(pkg, contigs, refs, [], o, kern_of(pkg, kernel))
        eng.set_regions(*rl.to_arrays(ivs))
        eng.submit(tl.raw_records(refs, recs))
        fin, tot = eng.finish_site_context(), eng.finish()
        eng.close()
        check_split(tot, fin, want_in, want_out, (kernel, n))
        assert fin[0][2:].sum() > 50


# ---- rules -----------------------------------------------------------------------------------------------------------

def test_rules(pkg):
    E = pkg.PssbamError
    eng = pkg.Engine(pss=dict(region_len=5))
    with pytest.raises(E):                                  # an unknown mode
        eng.set_site_context(2)
    with pytest.raises(E):
        eng.set_site_context(-1)
    with pytest.raises(ValueError):
        eng.set_site_context("chh")
    with pytest.raises(E):                                  # off: nothing to finish
        eng.finish_site_context()
    eng.set_site_context(None)                              # off stays off
    assert eng.site_context is None and eng.counters_device()[1] == eng.counter_layout()["n_u64"]
    eng.close()
    for cfg in (dict(kmer=dict(klen=4)), dict(pss=dict(region_len=5), kmer=dict(klen=4))):
        with pytest.raises(E):                              # PSSBAM_TALLY_KMER in the mask
            pkg.Engine(site_context="cpg", **cfg)
    for other in (dict(read_groups=["a"]), dict(length_bins=[30]), dict(contig_sets={"x": ["chrA"]}), dict(length_hist=100)):
        eng = pkg.Engine(pss=dict(region_len=5), **other)
        with pytest.raises(E):                              # planes or histogram set: no site context
            eng.set_site_context("cpg")
        assert eng.site_context is None
        eng.close()
    eng = pkg.Engine(pss=dict(region_len=5), site_context="cpg")
    for setter, arg in ((eng.set_read_groups, ["a"]), (eng.set_length_bins, [30]), (eng.set_contig_sets, {"x": ["chrA"]}),
                        (eng.set_length_histogram, 100)):
        with pytest.raises(E):                              # and the other way round
            setter(arg)
    assert eng.site_context == "cpg" and eng.read_groups == [] and eng.length_bins == [] and eng.contig_sets == [] and eng.length_hist == 0
    eng.set_site_context("none")                            # off again: the planes are legal, the pair is gone
    with pytest.raises(E):
        eng.finish_site_context()
    eng.set_length_bins([30])
    eng.close()

    eng = pkg.Engine(pss=dict(region_len=5), read_group="grpA", min_base_qual=10, site_context="cpg")   # goes with -R and -Q
    lay = eng.counter_layout()
    assert lay["site_fwd"] == lay["stats"] + pkg.ST_N == 2 * 7 * 16 + pkg.ST_N and lay["site_rev"] == lay["site_fwd"] + 7 * 16
    assert lay["n_u64"] == lay["site_rev"] + 7 * 16 == eng.counters_device()[1]
    contigs, refs, recs = tl.fuzz_dataset(5, 300, with_rg=True)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    for m in ("cpg", None):
        with pytest.raises(E):                              # records have been tallied
            eng.set_site_context(m)
    first = eng.finish_site_context()
    assert first[0][2:].sum() > 0
    eng.reset()                                             # the setting survives reset
    assert eng.counters_device()[1] == lay["n_u64"]
    zf, zr = eng.finish_site_context()
    assert not zf.any() and not zr.any()
    eng.submit(tl.raw_records(refs, recs))
    again = eng.finish_site_context()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    eng.reset()
    eng.set_site_context(None)                              # legal again after reset
    assert eng.counters_device()[1] == eng.counter_layout()["n_u64"] == lay["site_fwd"]
    eng.close()

    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_site_context("cpg")
    eng.close()
    other.close()


def test_bound_counters_receive_the_pair(pkg, fuzz):
    """a caller's block of the reported size (here: a second engine's own block) receives fwd_in | rev_in at the
    offsets counter_layout() documents, rows 0 and 1 zero; read back raw, as a caller that sums blocks would see it"""
    contigs, refs, recs, sams, g = fuzz
    o = tl.PssOpts(region_len=40)
    want, want_in = tables_of(pkg, contigs, refs, recs, o, pkg.KERNEL_TILED)
    eng, owner = pkg.Engine(pss=pss_dict(o), site_context="cpg"), pkg.Engine(pss=pss_dict(o), site_context="cpg")
    lay = eng.counter_layout()
    d, n = owner.counters_device()
    assert n == lay["n_u64"] == eng.counters_device()[1]
    owner.sync()                                            # the block is zeroed
    eng.bind_counters(d, n)
    assert eng.counters_device() == (d, n)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    got = eng.finish()
    host = np.zeros(n, dtype=np.uint64)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(host.ctypes.data, d, host.nbytes, 2) == 0      # hipMemcpyDeviceToHost
    eng.close()
    owner.close()
    cells = 42 * 16
    for key, w in (("site_fwd", want_in[0]), ("site_rev", want_in[1])):
        raw = host[lay[key]:lay[key] + cells].reshape(-1, 16)
        assert not raw[:2].any() and np.array_equal(raw[2:], w[2:]), key
    assert np.array_equal(host[:lay["rev"]].reshape(-1, 16), want.fwd) and np.array_equal(got.fwd, want.fwd)
    assert int(host[lay["stats"] + pkg.ST_NAMES.index("pss_ok")]) == want.stats["pss_ok"]


def test_submit_bgzf_set_after_feed_open(pkg, oracle, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(9403, 4000)
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    o = tl.PssOpts(region_len=31, min_mq=5)
    want_in, want_out = masked_oracle(oracle, tmp_path, contigs, refs, recs, o)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_site_context("cpg")
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    fin, tot = eng.finish_site_context(), eng.finish()
    assert eng.feed_status()["flags"] == 0 and tot.stats["records"] == len(recs)
    eng.close()
    check_split(tot, fin, want_in, want_out)
    assert fin[0][2:].sum() > 100


# ---- the command line ----------------------------------------------------------------------------------------------

def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


@pytest.fixture(scope="module")
def cli_case(oracle, tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(9404, 6000)
    recs = tl.ref_safe(recs)
    d = tmp_path_factory.mktemp("site_cli")
    o = tl.PssOpts(region_len=40, min_mq=10)
    want = masked_oracle(oracle, d, contigs, refs, recs, o)
    return contigs, refs, recs, o, want


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_X(pkg, cli_case, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    contigs, refs, recs, o, (want_in, want_out) = cli_case
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, contigs)
    aln = tmp_path / f"in.{fmt}"
    write_aln(aln, fmt, refs, recs)
    env = {**os.environ, **extra}

    def run(aln_path, out, *more):
        return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln_path), "-o", str(out), *more] + o.argv(), capture_output=True,
                              text=True, env=env, timeout=300)

    pr = run(aln, tmp_path / "out", "-X", "cpg")
    assert pr.returncode == 0, pr.stderr
    assert pr.stderr.splitlines()[0].endswith(" -X cpg")
    assert sorted(p.name for p in tmp_path.glob("out.*")) == sorted(
        [f"out.pss.{k}.txt" for k in ("counts", "rates")] + [f"out.{t}.pss.{k}.txt" for t in ("cpg", "noncpg") for k in ("counts", "rates")])
    pr = run(aln, tmp_path / "plain")
    assert pr.returncode == 0, pr.stderr
    assert sorted(p.name for p in tmp_path.glob("plain.*")) == ["plain.pss.counts.txt", "plain.pss.rates.txt"]
    for kind in ("counts", "rates"):    # the plain pair: byte-identical to the run without -X
        assert (tmp_path / f"plain.pss.{kind}.txt").read_bytes().replace(b"plain.pss", b"out.pss") == (tmp_path / f"out.pss.{kind}.txt").read_bytes()
    for tag, want, keep in (("cpg", want_in, True), ("noncpg", want_out, False)):
        gf, gr = tl.parse_counts_text((tmp_path / f"out.{tag}.pss.counts.txt").read_text())
        assert np.array_equal(gf, want[0]) and np.array_equal(gr, want[1]), tag
        assert gf[2:].sum() > 500
        if tl.have_ref() and mode in ("bam_device_feed", "sam"):
            masked = tmp_path / f"masked_{tag}.{fmt}"
            write_aln(masked, fmt, refs, sc.mask_recs(contigs, recs, keep))
            _, _, wc, wr, _ = tl.run_ref_pss(fa, masked, tmp_path / f"ref_{tag}", o, bam2sam=str(exe.parent / "bam2sam"), timeout=300)
            assert report_body(wc) == report_body((tmp_path / f"out.{tag}.pss.counts.txt").read_text()), tag
            assert report_body(wr) == report_body((tmp_path / f"out.{tag}.pss.rates.txt").read_text()), tag

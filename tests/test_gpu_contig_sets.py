"""pss-bam -C on the GPU: one set of substitution tables per set of reference sequences in one pass over the
records.  Every set's tables must equal what the reference computes with a FASTA holding only that set's contigs
(the CPU oracle on the reduced genome; for the command line also the same binary run with the reduced FASTA, and
the reference itself when oracle/_ref exists), the sets plus the unassigned bucket must sum to the totals, and
the totals must equal a run without sets."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

KERNELS = {"AUTO": 0, "SIMPLE": 1, "TILED": 2}


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq,
                up_ctx=o.up_ctx, down_ctx=o.down_ctx, merged_only=o.merged_only)


def oracle_sets(oracle, contigs, sam: Path, o: tl.PssOpts, sets: dict) -> dict:
    """{label: (fwd, rev)} of the oracle on the genome reduced to the label's contigs"""
    out = {}
    rows = o.region_len + 2
    for label, names in sets.items():
        keep = [c for c in contigs if c[0] in names]
        if not keep:
            out[label] = (np.zeros((rows, 16), dtype=np.uint64), np.zeros((rows, 16), dtype=np.uint64))
            continue
        g = oracle.genome_from_arrays(tl.loaded_contigs(keep))
        try:
            f, r, _ = oracle.pss(g, sam, o)
        finally:
            oracle.free_genome(g)
        out[label] = (f, r)
    return out


def plane0(eng):
    fwd = np.ones((eng.region_len + 2, 16), dtype=np.uint64)
    rev = np.ones_like(fwd)
    assert eng._L.pssbam_engine_finish_groups(eng._h, -1, fwd.ctypes.data, rev.ctypes.data) == 0
    return fwd, rev


def run_engine(pkg, contigs, refs, raw, o: tl.PssOpts, kernel, sets=None):
    eng = pkg.Engine(pss=pss_dict(o), kernel=kernel, read_group=o.read_group, contig_sets=sets)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(raw)
    return eng


def check_sets(pkg, oracle, contigs, refs, recs, sam, o, sets, kernel, raw=None):
    """sets == oracle on the reduced genome, sets + plane 0 == totals, totals == a run without sets"""
    raw = tl.raw_records(refs, recs) if raw is None else raw
    want = oracle_sets(oracle, contigs, sam, o, sets)
    eng = run_engine(pkg, contigs, refs, raw, o, kernel, sets)
    got = eng.finish_sets()
    assert list(got) == list(sets)
    for key, (wf, wr) in want.items():
        assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), (key, o)
    tot = eng.finish()
    p0f, p0r = plane0(eng)
    assert np.array_equal(sum(t.fwd for t in got.values()) + p0f, tot.fwd)
    assert np.array_equal(sum(t.rev for t in got.values()) + p0r, tot.rev)
    eng.close()
    plain = run_engine(pkg, contigs, refs, raw, o, kernel)
    ref_tot = plain.finish()
    plain.close()
    assert np.array_equal(tot.fwd, ref_tot.fwd) and np.array_equal(tot.rev, ref_tot.rev)
    drop = ("slow_path",)
    assert {k: v for k, v in tot.stats.items() if k not in drop} == {k: v for k, v in ref_tot.stats.items() if k not in drop}
    return got, tot


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    contigs, refs, recs = tl.fuzz_dataset(7201, 3000, contig_lens=(5000, 1200, 300, 900))
    sam = tmp_path_factory.mktemp("ctgsets") / "all.sam"
    tl.write_sam(sam, refs, recs)
    return contigs, refs, recs, sam


# chrB + a header name the FASTA lacks, chrA alone, two small contigs; scaffold_10 stays unassigned (plane 0)
SETS = {"big": ["chrB", "chrMissing"], "chrA": ["chrA"], "small": ["tiny.4", "nowhere"]}


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_engine_sets_match_oracle(pkg, oracle, fuzz, kernel):
    contigs, refs, recs, sam = fuzz
    rng = np.random.default_rng(300 + KERNELS[kernel])
    got, _ = check_sets(pkg, oracle, contigs, refs, recs, sam, tl.PssOpts(region_len=15), SETS, KERNELS[kernel])
    assert got["big"].fwd.sum() > 0 and got["chrA"].fwd.sum() > 0 and got["small"].rev.sum() > 0
    for n in (15, 25):
        o = tl.random_pss_opts(rng)
        o.region_len = n
        check_sets(pkg, oracle, contigs, refs, recs, sam, o, SETS, KERNELS[kernel])


def _many_refs_dataset(seed):
    """210 header names; the six real contigs at refIDs 0, 63, 64, 65, 199, 130 and one FASTA contig named "*" that
    receives the refID -1 records"""
    contigs, _, recs = tl.fuzz_dataset(seed, 4000, contig_lens=(5000, 1200, 300, 900, 700, 2500))
    refs = [(f"unplaced_{i:03d}", 1000 + i) for i in range(210)]
    for (nm, s), k in zip(contigs, [0, 63, 64, 65, 199, 130]):
        refs[k] = (nm, len(s))
    refs[7] = ("chrMissing", 4000)   # every RNAME must be a header name: a BAM writes any other one as refID -1
    rng = np.random.default_rng(seed)
    contigs = contigs + [("*", tl.random_contig(rng, 3000))]
    for r in recs:
        if r.rname == "*" and r.pos > 0:
            r.pos = min(r.pos, 2000)
        elif rng.random() < 0.03:
            r.rname = "unplaced_100"
    return contigs, refs, recs


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_engine_sets_past_64_references(pkg, oracle, tmp_path, kernel):
    """sets mix refIDs below and above REF_LDS_ENTRIES (LDS-cached and global ref_info) and the "*" entry"""
    contigs, refs, recs = _many_refs_dataset(7202)
    sam = tmp_path / "a.sam"
    tl.write_sam(sam, refs, recs)
    names = [nm for nm, _ in contigs]
    sets = {"lo_hi": [names[0], names[2]], "mid": [names[1], names[3], names[4]], "star": ["*", "unplaced_100"]}
    o = tl.PssOpts(region_len=20)
    got, _ = check_sets(pkg, oracle, contigs, refs, recs, sam, o, sets, KERNELS[kernel])
    assert all(got[k].fwd.sum() + got[k].rev.sum() > 0 for k in sets)


def test_engine_sets_overflow_path(pkg, oracle, fuzz, monkeypatch):
    """records longer than the staged prefix take the one-lane contig-set path"""
    monkeypatch.setenv("PSSBAM_TILE_READS", "64")
    monkeypatch.setenv("PSSBAM_PIECES", "5")
    contigs, refs, recs, sam = fuzz
    for n in (15, 40):
        _, tot = check_sets(pkg, oracle, contigs, refs, recs, sam, tl.PssOpts(region_len=n), SETS, pkg.KERNEL_TILED)
        assert tot.stats["slow_path"] > 0


@pytest.mark.parametrize("n", [15, 40])
def test_engine_sets_plane_and_row_passes(pkg, oracle, fuzz, monkeypatch, n):
    """5 sets with PSSBAM_GROUP_SLOTS=2: several plane passes; -r 40: a later row pass"""
    contigs, refs, recs, sam = fuzz
    sets = {"s0": ["chrB"], "s1": ["chrA"], "s2": ["scaffold_10"], "s3": ["tiny.4"], "s4": ["chrMissing"]}
    monkeypatch.setenv("PSSBAM_GROUP_SLOTS", "2")
    check_sets(pkg, oracle, contigs, refs, recs, sam, tl.PssOpts(region_len=n, min_mq=5), sets, pkg.KERNEL_TILED)


@pytest.mark.parametrize("kernel", ["TILED", "SIMPLE"])
def test_engine_sets_of_one_read_group(pkg, oracle, kernel, tmp_path):
    """-C with -R: the sets of the records -R keeps"""
    contigs, refs, recs = tl.fuzz_dataset(7203, 3000, with_rg=True)
    keep = [r for r in recs if ("RG", "Z", "grpA") in r.tags]
    sam = tmp_path / "keep.sam"
    tl.write_sam(sam, refs, keep)
    o = tl.PssOpts(region_len=25)
    want = oracle_sets(oracle, contigs, sam, o, SETS)
    o_rg = tl.PssOpts(**{**pss_dict(o), "read_group": "grpA"})
    eng = run_engine(pkg, contigs, refs, tl.raw_records(refs, recs), o_rg, KERNELS[kernel], SETS)
    got = eng.finish_sets()
    for key, (wf, wr) in want.items():
        assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), key
    assert eng.finish().stats["rg_dropped"] == len(recs) - len(keep)
    eng.close()


def test_engine_sets_rules(pkg, oracle, fuzz):
    E = pkg.PssbamError
    contigs, refs, recs, sam = fuzz
    with pytest.raises(E):                                  # k-mer tables are not split
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), contig_sets={"x": ["chrA"]})
    with pytest.raises(E):                                  # read groups set
        pkg.Engine(pss=dict(region_len=5), read_groups=["a"], contig_sets={"x": ["chrA"]})
    with pytest.raises(E):                                  # length bins set
        pkg.Engine(pss=dict(region_len=5), length_bins=[30], contig_sets={"x": ["chrA"]})
    eng = pkg.Engine(pss=dict(region_len=5), contig_sets={"x": ["chrA"]})
    for other in (lambda: eng.set_read_groups(["a"]), lambda: eng.set_length_bins([30])):
        with pytest.raises(E):                              # and the other way round
            other()
    for bad in ({}, [("chrA", "x"), ("chrA", "y")], [(f"c{i}", f"l{i}") for i in range(4097)]):
        with pytest.raises(E):
            eng.set_contig_sets(bad)
    L = eng._L
    import ctypes as C
    names, set_of = (C.c_char_p * 1)(b"chrA"), (C.c_int32 * 1)(1)
    assert L.pssbam_engine_set_contig_sets(eng._h, 1, 1, names, set_of) == -1   # set_of out of range
    assert L.pssbam_engine_set_contig_sets(eng._h, 0, 1, names, set_of) == -1
    assert eng.contig_sets == ["x"]
    eng.set_contig_sets([("chrA", "x"), ("chrA", "x")])   # the same name under the same set: harmless
    eng.close()
    o = tl.PssOpts(region_len=15)
    want = oracle_sets(oracle, contigs, sam, o, SETS)
    raw = tl.raw_records(refs, recs)

    def same(got):
        return all(np.array_equal(got[k].fwd, want[k][0]) and np.array_equal(got[k].rev, want[k][1]) for k in want)

    # set after set_references: the reference table is packed again
    eng = pkg.Engine(pss=pss_dict(o))
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.set_contig_sets(SETS)
    eng.submit(raw)
    assert same(eng.finish_sets())
    with pytest.raises(E):                                  # records have been tallied
        eng.set_contig_sets(SETS)
    eng.reset()                                             # the sets survive reset
    assert eng.contig_sets == list(SETS)
    eng.submit(raw)
    assert same(eng.finish_sets())
    eng.reset()
    eng.set_contig_sets({"only": ["chrA"]})                 # legal again after reset, and replaces the map
    eng.submit(raw)
    assert np.array_equal(eng.finish_sets()["only"].fwd, want["chrA"][0])
    eng.close()
    # set before set_genome; a later set_references (e.g. a longer list) applies them again
    eng = pkg.Engine(pss=pss_dict(o), contig_sets=[(nm, lab) for lab, nms in SETS.items() for nm in nms])
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs][:2])
    eng.set_references([nm for nm, _ in refs])
    eng.submit(raw)
    assert same(eng.finish_sets())
    lay = eng.counter_layout()
    assert [x["label"] for x in lay["contig_sets"]] == list(SETS) and lay["n_u64"] == eng.counters_device()[1]
    eng.close()
    eng, other = pkg.Engine(pss=dict(region_len=5)), pkg.Engine(pss=dict(region_len=5))
    d, n = other.counters_device()
    eng.bind_counters(d, n)
    with pytest.raises(E):                                  # a bound counter block cannot grow
        eng.set_contig_sets(SETS)
    eng.close()
    other.close()


def test_submit_bgzf_sets_set_after_feed_open(pkg, oracle, tmp_path):
    contigs, refs, recs = tl.fuzz_dataset(7204, 4000, contig_lens=(5000, 1200, 300, 900))
    bam = tmp_path / "x.bam"
    hb = tl.write_bam_aligned(bam, refs, recs, rng=np.random.default_rng(3))
    sam = tmp_path / "all.sam"
    tl.write_sam(sam, refs, recs)
    o = tl.PssOpts(region_len=15, min_mq=5)
    want = oracle_sets(oracle, contigs, sam, o, SETS)
    eng = pkg.Engine(pss=pss_dict(o))
    eng.feed_open(len(refs))
    eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
    eng.set_contig_sets(SETS)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    got = eng.finish_sets()
    for key, (wf, wr) in want.items():
        assert np.array_equal(got[key].fwd, wf) and np.array_equal(got[key].rev, wr), key
    assert eng.feed_status()["flags"] == 0
    assert eng.finish().stats["records"] == len(recs)
    eng.close()


# ---- the command line ----------------------------------------------------------------------------------------------

CLI_MODES = {
    "bam_device_feed": ("bam", {}),
    "bam_host_reader": ("bam", {"PSSBAM_DEVICE_INFLATE": "0"}),
    "sam": ("sam", {}),
    "bam_two_gpus": ("bam", {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}),
}

# label -> contigs; "a/b x" needs %XX in its file name, "ghost" names no contig of the header or the FASTA
CLI_SETS = {"chrB": ["chrB"], "a/b x": ["chrA", "tiny.4"], "ghost": ["chrGhost"]}


@pytest.mark.parametrize("mode", list(CLI_MODES))
def test_cli_C_matches_reduced_fasta_per_set(pkg, mode, tmp_path):
    fmt, extra = CLI_MODES[mode]
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    contigs, refs, recs = tl.fuzz_dataset(7205, 6000, contig_lens=(5000, 1200, 300, 900))
    recs = tl.ref_safe(recs)
    run = tmp_path / "run"
    run.mkdir()
    tl.write_fasta(run / "g.fa", contigs)
    aln = tmp_path / f"in.{fmt}"
    if fmt == "bam":
        tl.write_bam(aln, refs, recs, rng=np.random.default_rng(2))
    else:
        tl.write_sam(aln, refs, recs)
    (tmp_path / "map.tsv").write_text("# label map\n" + "".join(f"{nm}\t{lab}\n" for lab, nms in CLI_SETS.items() for nm in nms)
                                      .replace("chrB\tchrB\n", "chrB\r\n"))
    o = tl.PssOpts(region_len=25, min_mq=10, min_read_len=10)
    env = {**os.environ, **extra}

    def pss_bam(cwd: Path, prefix: str, *more):
        pr = subprocess.run([str(exe), "-F", "g.fa", "-B", str(aln), "-o", prefix, *more] + o.argv(), capture_output=True,
                            text=True, env=env, timeout=300, cwd=cwd)
        assert pr.returncode == 0, pr.stderr
        return pr

    pr = pss_bam(run, "out", "-C", str(tmp_path / "map.tsv"))
    assert pr.stderr.splitlines()[0].endswith(f" -C {tmp_path / 'map.tsv'}")
    warn = [ln for ln in pr.stderr.splitlines() if ln.startswith("Warning: -C")]
    assert len(warn) == 1 and "ghost" in warn[0], pr.stderr
    tags = {"chrB": "chrB", "a/b x": "a%2Fb%20x", "ghost": "ghost"}
    files = {lab: ((run / f"out.{t}.pss.counts.txt").read_text(), (run / f"out.{t}.pss.rates.txt").read_text())
             for lab, t in tags.items()}
    assert len(list(run.glob("out.*.txt"))) == 2 * (len(CLI_SETS) + 1)
    tot_c, tot_r = (run / "out.pss.counts.txt").read_text(), (run / "out.pss.rates.txt").read_text()
    # the totals: byte-identical to the same command without -C
    plain = tmp_path / "plain"
    plain.mkdir()
    (plain / "g.fa").write_bytes((run / "g.fa").read_bytes())
    pss_bam(plain, "out")
    assert (plain / "out.pss.counts.txt").read_text() == tot_c and (plain / "out.pss.rates.txt").read_text() == tot_r
    # every set: byte-identical to this binary with the FASTA reduced to the set's contigs (same relative -F name)
    use_ref = tl.have_ref() and mode in ("bam_device_feed", "sam")
    sum_f = sum_r = 0
    for lab, (ct, rt) in files.items():
        d = tmp_path / f"set_{tags[lab]}"
        d.mkdir()
        keep = [c for c in contigs if c[0] in CLI_SETS[lab]]
        tl.write_fasta(d / "g.fa", keep if keep else [("unrelated", contigs[-1][1])])
        pss_bam(d, f"out.{tags[lab]}")
        assert (d / f"out.{tags[lab]}.pss.counts.txt").read_text() == ct, lab
        assert (d / f"out.{tags[lab]}.pss.rates.txt").read_text() == rt, lab
        if use_ref:
            cwd = os.getcwd()
            os.chdir(d)
            try:
                _, _, wc, wr, _ = tl.run_ref_pss(Path("g.fa"), aln, Path(f"out.{tags[lab]}"), o,
                                                 bam2sam=str(exe.parent / "bam2sam"), timeout=300)
            finally:
                os.chdir(cwd)
            assert wc == ct and wr == rt, lab
        f, r = tl.parse_counts_text(ct)
        sum_f, sum_r = sum_f + f, sum_r + r
        if lab == "ghost":
            assert not f.any() and not r.any()
    tf, trv = tl.parse_counts_text(tot_c)
    # scaffold_10 is in no set: the sets hold less than the totals, never more
    assert (tf >= sum_f).all() and (trv >= sum_r).all() and (tf > sum_f).any()

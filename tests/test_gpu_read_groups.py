"""pss-bam -G on the GPU: one set of substitution tables per @RG ID in one pass over the records.
Every group's tables must equal what -R <ID> gives (the CPU oracle on the records whose FIRST RG:Z is
that ID; the reference itself for the command line when oracle/_ref exists), the totals must equal an
ungrouped run, and the unassigned bucket (no RG:Z, or an ID the header lacks) is the rest."""
import gzip
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

IDS = ["grpA", "grpB", "a/b", ".", "x%y", "lib_5", "L6"]   # 7 groups = 8 planes: one pass


@pytest.fixture(scope="module")
def pkg():
    return ge.load_pkg()


def first_rg(r: tl.Rec):
    for tag, typ, val in r.tags:
        if tag == "RG" and typ == "Z":
            return val
    return None


def rg_dataset(seed: int, ids: list[str], n_reads: int = 3000, second_rg: bool = True):
    """fuzz_dataset(with_rg=True) (aux fields of every type, RGZ decoys in Z values and B arrays) with the RG:Z
    values rewritten over `ids`, records without RG, values no header line declares and a second RG:Z behind
    the first"""
    contigs, refs, recs = tl.fuzz_dataset(seed, n_reads, with_rg=True)
    rng = np.random.default_rng(seed + 1000)
    for r in recs:
        tags = [t for t in r.tags if not (t[0] == "RG" and t[1] == "Z")]
        u = rng.random()
        if u < 0.08:
            val = None                                           # no RG at all
        elif u < 0.14:
            val = "notInHeader"
        else:
            val = ids[int(rng.integers(0, len(ids)))]
        if val is not None:
            tags.insert(int(rng.integers(0, len(tags) + 1)), ("RG", "Z", val))
            if second_rg and rng.random() < 0.05:
                tags.append(("RG", "Z", ids[0] if val != ids[0] else ids[-1]))   # only the first one counts
        r.tags = tags
    return contigs, refs, recs


def header_text(refs, ids) -> str:
    h = "@HD\tVN:1.6\tSO:unknown\n" + "".join(f"@SQ\tSN:{n}\tLN:{l}\n" for n, l in refs)
    h += "".join(f"@RG\tID:{i}\tSM:s{k}\r\n" if k % 3 == 1 else f"@RG\tSM:s{k}\tID:{i}\n" for k, i in enumerate(ids))
    return h + f"@RG\tID:{ids[0]}\tSM:dup\n@CO\tend\n"


def write_sam(path: Path, refs, recs, ids):
    with open(path, "w") as fh:
        fh.write(header_text(refs, ids))
        for r in recs:
            fh.write(tl.sam_line(r))


def write_bam(path: Path, refs, recs, ids, rng) -> int:
    """BGZF BAM whose records cross block boundaries; returns the inflated header bytes"""
    hdr = header_text(refs, ids)
    raw = tl.bam_bytes(refs, recs, hdr)
    with open(path, "wb") as fh:
        i = 0
        while i < len(raw):
            n = int(rng.integers(1, 0xFF00))
            fh.write(tl.bgzf_block(raw[i:i + n], 1))
            i += n
        fh.write(tl.BGZF_EOF)
    return len(tl.bam_bytes(refs, [], hdr))


def pss_dict(o: tl.PssOpts) -> dict:
    return dict(region_len=o.region_len, min_read_len=o.min_read_len, max_read_len=o.max_read_len, min_mq=o.min_mq,
                up_ctx=o.up_ctx, down_ctx=o.down_ctx, merged_only=o.merged_only)


def oracle_by_group(oracle, g, refs, recs, ids, o, tmp_path):
    """{ID or None: (fwd, rev)} from the CPU oracle on each group's records"""
    out = {}
    for key in ids + [None]:
        sel = [r for r in recs if (first_rg(r) == key if key is not None else first_rg(r) not in ids)]
        sam = tmp_path / "grp.sam"
        tl.write_sam(sam, refs, sel)
        f, r, _ = oracle.pss(g, sam, o)
        out[key] = (f, r)
    return out


def check_engine(eng, want, ids):
    got = eng.finish_groups()
    assert set(got) == set(ids) | {None}
    for key in ids + [None]:
        assert np.array_equal(got[key].fwd, want[key][0]) and np.array_equal(got[key].rev, want[key][1]), key
    return got


@pytest.mark.parametrize("kernel", ["AUTO", "SIMPLE"])
def test_engine_groups_match_oracle(pkg, oracle, kernel, tmp_path):
    contigs, refs, recs = rg_dataset(11, IDS)
    raw = tl.raw_records(refs, recs)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    rng = np.random.default_rng(5)
    for n in (0, 15, 25, 40):
        o = tl.random_pss_opts(rng)
        o.region_len = n
        kern = pkg.KERNEL_AUTO if kernel == "AUTO" else pkg.KERNEL_SIMPLE
        eng = pkg.Engine(pss=pss_dict(o), kernel=kern, read_groups=IDS)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        eng.submit(raw)
        want = oracle_by_group(oracle, g, refs, recs, IDS, o, tmp_path)
        got = check_engine(eng, want, IDS)
        tot = eng.finish()
        eng.close()
        plain = pkg.Engine(pss=pss_dict(o), kernel=kern)
        plain.set_genome_arrays(tl.loaded_contigs(contigs))
        plain.set_references([nm for nm, _ in refs])
        plain.submit(raw)
        ref_tot = plain.finish()
        plain.close()
        assert np.array_equal(tot.fwd, ref_tot.fwd) and np.array_equal(tot.rev, ref_tot.rev), n
        assert tot.stats == ref_tot.stats or {k: v for k, v in tot.stats.items() if k != "slow_path"} == \
            {k: v for k, v in ref_tot.stats.items() if k != "slow_path"}
        # total minus the groups is the unassigned bucket
        rest_f = tot.fwd - sum(got[i].fwd for i in IDS)
        rest_r = tot.rev - sum(got[i].rev for i in IDS)
        assert np.array_equal(rest_f, want[None][0]) and np.array_equal(rest_r, want[None][1])
    oracle.free_genome(g)


def test_engine_groups_rules(pkg):
    with pytest.raises(pkg.PssbamError):
        pkg.Engine(pss=dict(region_len=5), read_group="grpA", read_groups=["grpA"])
    with pytest.raises(pkg.PssbamError):
        pkg.Engine(pss=dict(region_len=5), kmer=dict(klen=4), read_groups=["grpA"])
    eng = pkg.Engine(pss=dict(region_len=5))
    with pytest.raises(pkg.PssbamError):
        eng.set_read_groups([])
    eng.set_read_groups(["a", "b"])
    lay = eng.counter_layout()
    assert [x["id"] for x in lay["groups"]] == ["a", "b"] and lay["n_u64"] == eng.counters_device()[1]
    contigs, refs, recs = rg_dataset(3, ["a", "b"], 200)
    eng.set_genome_arrays(tl.loaded_contigs(contigs))
    eng.set_references([nm for nm, _ in refs])
    eng.submit(tl.raw_records(refs, recs))
    with pytest.raises(pkg.PssbamError):       # records have been tallied
        eng.set_read_groups(["a"])
    eng.reset()
    eng.set_read_groups(["a"])                  # legal again after reset
    eng.close()


@pytest.mark.parametrize("n_groups", [7, 40])
def test_submit_bgzf_groups_set_after_feed_open(pkg, oracle, n_groups, tmp_path):
    ids = IDS if n_groups == 7 else [f"g{k:02d}" for k in range(38)] + ["a/b", "."]
    contigs, refs, recs = rg_dataset(23 + n_groups, ids, 4000)
    bam = tmp_path / "x.bam"
    hb = write_bam(bam, refs, recs, ids, np.random.default_rng(n_groups))
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    for n in ((15, 40) if n_groups == 7 else (25,)):
        o = tl.PssOpts(region_len=n, min_mq=5)
        eng = pkg.Engine(pss=pss_dict(o))
        eng.feed_open(len(refs))
        eng.submit_bgzf(np.frombuffer(bam.read_bytes(), dtype=np.uint8), header_bytes=hb, max_batch_inflated=70000)
        eng.set_read_groups(ids)
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([nm for nm, _ in refs])
        want = oracle_by_group(oracle, g, refs, recs, ids, o, tmp_path)
        check_engine(eng, want, ids)
        assert eng.feed_status()["flags"] == 0
        tot = eng.finish()
        f_all, r_all, _ = oracle.pss(g, _all_sam(tmp_path, refs, recs), o)
        assert np.array_equal(tot.fwd, f_all) and np.array_equal(tot.rev, r_all)
        assert tot.stats["records"] == len(recs)
        eng.close()
    oracle.free_genome(g)


def _all_sam(tmp_path, refs, recs):
    p = tmp_path / "all.sam"
    tl.write_sam(p, refs, recs)
    return p


def _expected_group_files(oracle, g, fa, aln, prefix, refs, recs, o, key, tmp_path, use_ref, bam2sam):
    """(counts text, rates text) that `-R key -o <prefix>` writes: the reference when it is there, else the oracle"""
    if use_ref:
        _, _, ct, rt, _ = tl.run_ref_pss(fa, aln, prefix, tl.PssOpts(**{**pss_dict(o), "read_group": key}), bam2sam=bam2sam,
                                         timeout=300)
        return ct, rt
    sel = [r for r in recs if first_rg(r) == key]
    sam = tmp_path / "sel.sam"
    tl.write_sam(sam, refs, sel)
    f, r, _ = oracle.pss(g, sam, o)
    oracle.write_reports(str(fa), str(aln), str(prefix), f, r)
    return Path(f"{prefix}.pss.counts.txt").read_text(), Path(f"{prefix}.pss.rates.txt").read_text()


@pytest.mark.parametrize("fmt", ["bam", "sam", "sam.gz"])
def test_cli_G_matches_R_per_group(pkg, oracle, fmt, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    # (no second RG:Z here: the test stand-in for `samtools view -r` on SAM text keeps a record with ANY matching RG:Z field)
    contigs, refs, recs = rg_dataset(31, IDS, 6000, second_rg=False)
    recs = tl.ref_safe(recs)
    fa = tmp_path / "g.fa"
    tl.write_fasta(fa, contigs)
    aln = tmp_path / f"in.{fmt}"
    if fmt == "bam":
        write_bam(aln, refs, recs, IDS, np.random.default_rng(2))
    else:
        write_sam(tmp_path / "in.sam", refs, recs, IDS)
        if fmt == "sam.gz":
            aln.write_bytes(gzip.compress((tmp_path / "in.sam").read_bytes()))
    o = tl.PssOpts(region_len=25, min_mq=10)
    prefix = tmp_path / "out"
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    envs = [{}, {"PSSBAM_NGPU": "2", "PSSBAM_OVERSUBSCRIBE": "1", "PSSBAM_BATCH_BYTES": "1048576"}]
    for extra in envs:
        env = {**os.environ, **extra}
        pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), "-G"] + o.argv(), capture_output=True,
                            text=True, env=env, timeout=300)
        assert pr.returncode == 0, pr.stderr
        assert pr.stderr.splitlines()[0].endswith(" -G")
        tot_c, tot_r = Path(f"{prefix}.pss.counts.txt").read_text(), Path(f"{prefix}.pss.rates.txt").read_text()
        group_files = {}
        for key in IDS:
            tagged = str(prefix) + "." + "".join(c if c.isalnum() or c in "_-" else f"%{ord(c):02X}" for c in key)
            group_files[key] = (Path(f"{tagged}.pss.counts.txt").read_text(), Path(f"{tagged}.pss.rates.txt").read_text(), tagged)
        assert ".%2E.pss.counts.txt" in str(list(tmp_path.iterdir()))
        # the totals: byte-identical to the same command without -G
        pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix)] + o.argv(), capture_output=True, text=True,
                            env=env, timeout=300)
        assert pr.returncode == 0, pr.stderr
        assert Path(f"{prefix}.pss.counts.txt").read_text() == tot_c
        assert Path(f"{prefix}.pss.rates.txt").read_text() == tot_r
        # every group: byte-identical to -R <ID> -o <prefix>.<E>
        sum_f = sum_r = 0
        for key in IDS:
            ct, rt, tagged = group_files[key]
            wc, wr = _expected_group_files(oracle, g, fa, aln, tagged, refs, recs, o, key, tmp_path,
                                           tl.have_ref() and fmt != "sam.gz", str(exe.parent / "bam2sam"))
            assert ct == wc, key
            assert rt == wr, key
            f, r = tl.parse_counts_text(ct)
            sum_f, sum_r = sum_f + f, sum_r + r
        # the unassigned bucket gets no file; it is the total minus the groups
        tf, trv = tl.parse_counts_text(tot_c)
        sel = [r for r in recs if first_rg(r) not in IDS]
        sam = tmp_path / "rest.sam"
        tl.write_sam(sam, refs, sel)
        wf, wr_, _ = oracle.pss(g, sam, o)
        assert np.array_equal(tf - sum_f, wf) and np.array_equal(trv - sum_r, wr_)
    oracle.free_genome(g)


def test_cli_G_without_rg_header_writes_totals_only(pkg, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    contigs, refs, recs = tl.fuzz_dataset(4, 500)
    fa, sam = tmp_path / "g.fa", tmp_path / "a.sam"
    tl.write_fasta(fa, contigs)
    tl.write_sam(sam, refs, recs)
    pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(sam), "-o", str(tmp_path / "o"), "-G"], capture_output=True, text=True,
                        timeout=300)
    assert pr.returncode == 0, pr.stderr
    assert "Warning" in pr.stderr and "@RG" in pr.stderr
    assert sorted(p.name for p in tmp_path.glob("o.*")) == ["o.pss.counts.txt", "o.pss.rates.txt"]

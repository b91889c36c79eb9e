"""Pins the CPU restatement (oracle/liboracle.so) to the UNMODIFIED reference on randomised input.

The reference's outputs for these inputs are stored in tests/golden/fuzz_ref.npz (written by
tests/golden/make_golden.py from the oracle/_ref build); the inputs are regenerated here from their
seeds and must match the digest stored with each output, so the test needs no reference build.
"""
import numpy as np
import pytest

import pssbam_testlib as tl
from pssbam_testlib import PssOpts

REF_OUT = np.load(tl.FUZZ_REF)


def _stored_text(key: str) -> str:
    return REF_OUT[key].tobytes().decode()


def _check_inputs(key: str, files: list[str], opts=None):
    assert tl.inputs_digest(files, opts) == str(REF_OUT[key + "_inputs"]), \
        f"{key}: the generated inputs are not those the stored outputs came from (rerun tests/golden/make_golden.py)"


@pytest.mark.parametrize("seed", range(tl.FUZZ_SEEDS))
def test_pss_restatement_matches_reference(tmp_path, monkeypatch, oracle, seed):
    monkeypatch.chdir(tmp_path)
    fa, sam, opts = tl.pss_fuzz_case(seed)
    g = oracle.load_genome(fa)
    try:
        for trial, o in enumerate(opts):
            key = f"pss_{seed}_{trial}"
            _check_inputs(key, [fa, sam], o)
            ctext, rtext = _stored_text(key + "_counts"), _stored_text(key + "_rates")
            rf, rr = tl.parse_counts_text(ctext)
            fwd, rev, _ = oracle.pss(g, sam, o)
            assert np.array_equal(fwd, rf), f"fwd differs seed={seed} opts={o}"
            assert np.array_equal(rev, rr), f"rev differs seed={seed} opts={o}"
            # report writers: byte-exact files (same -F/-B/-o strings)
            oracle.write_reports(fa, sam, f"ref{trial}", fwd, rev)
            assert (tmp_path / f"ref{trial}.pss.counts.txt").read_text() == ctext
            assert (tmp_path / f"ref{trial}.pss.rates.txt").read_text() == rtext
    finally:
        oracle.free_genome(g)


def test_pss_counts_are_nontrivial(tmp_path, monkeypatch, oracle):
    """guards against a fuzz set that everything filters out of"""
    monkeypatch.chdir(tmp_path)
    fa, sam, _ = tl.pss_fuzz_case(77)
    g = oracle.load_genome(fa)
    fwd, rev, st = oracle.pss(g, sam, PssOpts(region_len=5))
    oracle.free_genome(g)
    assert st[0] > 100 and fwd.sum() > 500 and rev.sum() > 500
    assert st[1] > 0 and st[2] > 0 and st[3] > 0        # parse-skip, no-contig, filtered all occur


@pytest.mark.parametrize("seed", range(tl.FUZZ_SEEDS))
def test_fragkon_restatement_matches_reference(tmp_path, monkeypatch, oracle, seed):
    monkeypatch.chdir(tmp_path)
    fa, trials = tl.fk_fuzz_case(seed)
    g = oracle.load_genome(fa)
    try:
        for trial, (o, sam) in enumerate(trials):
            key = f"fk_{seed}_{trial}"
            _check_inputs(key, [fa, sam], o)
            k5, k3, _ = oracle.fragkon(g, sam, o)
            r5 = tl.dense(4 ** o.klen, REF_OUT[key + "_idx"], REF_OUT[key + "_k5"])
            r3 = tl.dense(4 ** o.klen, REF_OUT[key + "_idx"], REF_OUT[key + "_k3"])
            assert np.array_equal(k5, r5), f"5' differs seed={seed} opts={o}"
            assert np.array_equal(k3, r3), f"3' differs seed={seed} opts={o}"
    finally:
        oracle.free_genome(g)


def test_gz_fasta_and_O2_build_agree(tmp_path, monkeypatch, oracle):
    """the reference at its own flags on the plain FASTA and at -O2 on the gzipped one wrote the same
    tables; the restatement reads the gzipped FASTA to the same tables"""
    monkeypatch.chdir(tmp_path)
    fa, fagz, sam, o = tl.gz_fuzz_case()
    _check_inputs("gz", [fa, sam], o)
    a = tl.parse_counts_text(_stored_text("gz_counts"))
    b = tl.parse_counts_text(_stored_text("gz_counts_O2"))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    g = oracle.load_genome(fagz)
    fwd, rev, _ = oracle.pss(g, sam, o)
    oracle.free_genome(g)
    assert np.array_equal(fwd, a[0]) and np.array_equal(rev, a[1])


@pytest.mark.parametrize("k", tl.GKC_KS)
def test_genome_kmer_count_restatement_matches_reference(tmp_path, monkeypatch, oracle, k):
    monkeypatch.chdir(tmp_path)
    fa = tl.gkc_fuzz_case(k)
    _check_inputs(f"gkc_{k}", [fa])
    g = oracle.load_genome(fa)
    got = oracle.genome_kmer_count(g, k)
    oracle.free_genome(g)
    want = tl.dense(4 ** k, REF_OUT[f"gkc_{k}_idx"], REF_OUT[f"gkc_{k}_counts"])
    assert np.array_equal(got, want) and got.sum() > 20000

"""The yardstick of pss-bam -y / -Y, shared by test_read_score_host.py and test_gpu_read_score.py.

The read score S of a record (include/pssbam_hip.h, pssbam_engine_set_read_score) restated in plain Python, the
post-mortem-damage weight table from its formula, the reduced inputs the contract is written in -- the input without the
records whose S is defined and below the minimum, and the per-bin subsets of the histogram identities -- and makers of
hand-built records for the edge cases."""
from __future__ import annotations

import math
from pathlib import Path

import numpy as np

import pssbam_testlib as tl
from mismatch_lib import clean_contig, pss_length, read_on, read_sam  # noqa: F401  (re-exported)

ACGT = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
GOLD = Path(__file__).resolve().parent / "golden"
PMD_DIST, PMD_QUAL, PMD_HALF, PMD_SHIFT = 32, 64, 32, 8


def qual_bytes(rec: tl.Rec) -> list:
    """QUAL as the BAM record stores it: Phred values, 0xFF throughout where the text is '*'"""
    n = 0 if rec.seq == "*" else len(rec.seq)
    return [0xFF] * n if rec.qual == "*" else [ord(c) - 33 for c in rec.qual]


def score(rec: tl.Rec, contigs, W, min_bq: int = 0):
    """S of a record whose CIGAR is exactly <L>M on a contig of the FASTA; None where S is not defined.
    W: integers [4][n_dist][n_qual]; contigs: [(id, text)] as written (any case) or {id: text}."""
    ctg = contigs if isinstance(contigs, dict) else dict(contigs)
    L = pss_length(rec)
    if rec.cigar != [(L, "M")] or rec.rname not in ctg:
        return None
    W = np.asarray(W)
    n_dist, n_qual = W.shape[1], W.shape[2]
    g = ctg[rec.rname].upper()
    seq = "" if rec.seq == "*" else rec.seq.upper()
    qual = qual_bytes(rec)
    s = rec.pos - 1
    rev = bool(rec.flag & 0x10)
    S = 0
    for i in range(min(L, len(seq))):
        p = s + i
        if not 0 <= p < len(g):
            continue
        a, b = seq[i], g[p]
        if a not in ACGT or b not in ACGT:
            continue
        if min_bq and qual[i] < min_bq:
            continue
        if b == "C" and a in "CT":
            kind, d = (1 if a == "T" else 0), i
        elif b == "G" and a in "GA":
            kind, d = (3 if a == "A" else 2), L - 1 - i
        else:
            continue
        if rev:
            kind ^= 2
        S += int(W[kind][min(d, n_dist - 1)][min(qual[i], n_qual - 1)])
    return max(-2 ** 31, min(S, 2 ** 31 - 1))


def score_bin(S: int, half: int, shift: int) -> int:
    return max(-half, min(S >> shift, half - 1)) + half      # Python's >> floors, like an arithmetic shift


def reduce_to(recs, contigs, W, min_score: int, min_bq: int = 0) -> list:
    """the records without those whose S is defined and below min_score"""
    ctg = dict(contigs)
    out = []
    for r in recs:
        S = score(r, ctg, W, min_bq)
        if S is None or S >= min_score:
            out.append(r)
    return out


def split_by_bin(recs, contigs, W, half: int, shift: int, min_bq: int = 0) -> list:
    """[bin 0, ..., bin 2 * half - 1]: the records whose score bin it is (records without an S are in no bin)"""
    ctg = dict(contigs)
    bins: list = [[] for _ in range(2 * half)]
    for r in recs:
        S = score(r, ctg, W, min_bq)
        if S is not None:
            bins[score_bin(S, half, shift)].append(r)
    return bins


def reduce_sam_text(text: str, contigs, W, min_score: int) -> str:
    """the same reduction on SAM text: header lines and every kept record line pass through byte for byte"""
    ctg = dict(contigs)
    out = []
    for ln in text.splitlines(keepends=True):
        if not ln.startswith("@"):
            f = ln.rstrip("\n").split("\t")
            cigar = [(int(f[5][:-1]), "M")] if f[5][:-1].isdigit() and f[5].endswith("M") else [(0, "?")]
            r = tl.Rec(qname=f[0], flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=cigar, tlen=int(f[8]), seq=f[9], qual=f[10])
            S = score(r, ctg, W)
            if S is not None and S < min_score:
                continue
        out.append(ln)
    return "".join(out)


# ---- the post-mortem-damage table ------------------------------------------------------------------------------------

def pmd_formula() -> np.ndarray:
    """[4][32][64] floats, before rounding: 256 ln of the likelihood ratio, double-stranded model, default parameters"""
    pi, d_modern = 0.001, 0.001
    out = np.zeros((4, PMD_DIST, PMD_QUAL))

    def p_match(D, eps):
        return (1 - pi) * (1 - eps) * (1 - D) + (1 - pi) * eps * D + pi * eps * (1 - D)

    for z in range(PMD_DIST):
        d_ancient = 0.3 * 0.7 ** z + 0.01
        for q in range(PMD_QUAL):
            eps = 10 ** (-q / 10) / 3
            pa, pm = p_match(d_ancient, eps), p_match(d_modern, eps)
            out[0, z, q] = out[2, z, q] = 256 * math.log(pa / pm)
            out[1, z, q] = out[3, z, q] = 256 * math.log((1 - pa) / (1 - pm))
    return out


def committed_pmd_weights() -> np.ndarray:
    """tests/golden/pmd_weights.txt: the table the goldens were made with, [4][32][64], one row of 64 per line"""
    rows = [[int(x) for x in ln.split()] for ln in (GOLD / "pmd_weights.txt").read_text().splitlines() if ln and not ln.startswith("#")]
    W = np.array(rows, dtype=np.int64)
    assert W.shape == (4 * PMD_DIST, PMD_QUAL)
    return W.reshape(4, PMD_DIST, PMD_QUAL)


def random_weights(seed: int, n_dist: int, n_qual: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(-2047, 2048, size=(4, n_dist, n_qual)).astype(np.int16)


# ---- what the GPU tests run, fixed here so that test_read_score_host.py can show that none of it is vacuous --------------

FUZZ = (7301, 1000)      # tl.fuzz_dataset(seed, n_reads): 626 records with a score, 1 to 259 bases


def tables() -> dict:
    """the PMD table, the widest random table, the narrowest (one weight per kind), and one of small weights whose scores
    sit around zero (the unshifted four-bin histogram)"""
    return {"pmd": committed_pmd_weights(), "wide": random_weights(41, PMD_QUAL, 64), "narrow": np.array([[[700]], [[-1500]], [[-900]], [[2047]]], dtype=np.int16),
            "tiny": np.array([[[-1]], [[2]], [[1]], [[-2]]], dtype=np.int16)}


# (table, minimum base quality, minimum score): chosen from the distribution of `score` over the fuzz set so that each
# keeps between 20 % and 80 % of the records that have a score
CUTS = (("pmd", 0, -200), ("pmd", 0, -100), ("pmd", 20, -100), ("wide", 0, 0), ("wide", 0, 2000), ("narrow", 0, -1500))
# (table, hist_half, hist_shift)
HIST_SHAPES = (("tiny", 2, 0), ("pmd", 2, 8), ("pmd", 128, 0), ("wide", 128, 8))


# ---- hand-built records ----------------------------------------------------------------------------------------------

def revcomp_twin(rec: tl.Rec, rname: str, at: int) -> tl.Rec:
    """the record that holds the reverse complement of rec's read on the other strand, placed at 0-based `at` of contig `rname`,
    whose text there is the reverse complement of rec's reference stretch: same score by the definition"""
    seq = "".join(COMP.get(c, c) for c in reversed(rec.seq.upper()))
    qual = rec.qual if rec.qual == "*" else rec.qual[::-1]
    return tl.Rec(qname=rec.qname + "t", flag=rec.flag ^ 0x10, rname=rname, pos=at + 1, mapq=rec.mapq, cigar=list(rec.cigar),
                  tlen=rec.tlen, seq=seq, qual=qual)


def revcomp(text: str) -> str:
    return "".join(COMP.get(c, c) for c in reversed(text.upper()))


def with_qual(rec: tl.Rec, qual) -> tl.Rec:
    """rec with the given Phred values (a list) or '*'"""
    q = qual if qual == "*" else "".join(chr(33 + v) for v in qual)
    return tl.Rec(**{**rec.__dict__, "qual": q})

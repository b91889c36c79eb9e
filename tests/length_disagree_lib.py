"""Records whose SEQ, CIGAR and TLEN disagree, shared by test_length_disagree_host.py and test_gpu_length_disagree.py.

For a paired read pss-bam takes L = |TLEN|, and the read passes when its CIGAR is `<L>M`, however many bases SEQ holds.
Base k of the read is SEQ[k] where k < l_seq and no base at all (a non-ACGT code, precondition P3 of the oracle)
elsewhere, so the 3' window sits at SEQ[L-1-i], not at SEQ[l_seq-1-i].  The yardstick follows:

    a paired `<|TLEN|>M` record is tallied as if SEQ were cut to |TLEN| bases, or padded with N on the right up to
    |TLEN| bases.

`dataset` draws such records (two thirds of the set; the rest are ordinary tl.fuzz_dataset records so that every status
counter moves), `normalise` is the cut / pad, and `anchor_on_l_seq` / `unblanked` are two WRONG models that exist only
so the host test can show that the data tells them apart.  fragkon compares strlen(SEQ) with the CIGAR and filters a
disagreeing record; nothing here is normalised for it.  CPU only."""
from __future__ import annotations

from dataclasses import replace

import numpy as np

import pssbam_testlib as tl

# every nibble of these QUAL bytes is a BAM base code (1 2 4 8 = A C G T): a kernel that reads past SEQ into QUAL sees
# bases that change a cell instead of codes that vanish as non-ACGT.  17 and 18 are below -Q 20.
QUAL_VALUES = (17, 18, 20, 24, 33, 34, 36, 40)
ROW_PASSES = (7, 15, 16, 25, 40)        # the -r values of the tests: N of the SEQ lengths drawn relative to N
SEED, N_READS, REGION = 9701, 3200, 40   # the dataset both test files use: T >= 40, so every read reaches the second row pass of -r 40
CLASSES = ((0x40, 0), (0x40, 0x10), (0x80, 0), (0x80, 0x10))     # mate by strand


def crafted(recs: list) -> list:
    """the records `dataset` built itself (names d...), as opposed to the tl.fuzz_dataset third (names r...)"""
    return [r for r in recs if r.qname.startswith("d")]


def governed(r: tl.Rec) -> bool:
    """a paired record whose CIGAR is `<|TLEN|>M` with SEQ and QUAL both present or both absent: what normalise rewrites"""
    t = abs(r.tlen)
    return bool(r.flag & 1) and t >= 1 and r.cigar == [(t, "M")] and (r.seq == "*") == (r.qual == "*")


def kind(r: tl.Rec) -> str:
    """short / equal / long / star by the bases SEQ holds against |TLEN|"""
    if r.seq == "*":
        return "star"
    n, t = len(r.seq), abs(r.tlen)
    return "short" if n < t else "long" if n > t else "equal"


def _name(rng, i: int) -> str:
    """1 to 40 characters: with the SEQ lengths they put the records at every offset mod 16 of the record block"""
    body = "d" + np.base_repr(i, 36).lower()
    n = int(rng.integers(1, 41))
    return body[:n].ljust(n, "x")


def dataset(seed: int, n_reads: int, region_len: int, contig_lens=(5000, 1200, 300), with_rg: bool = False):
    """(contigs, refs, recs) on the genome of tl.fuzz_dataset(seed, ...).  About a third of the records are that
    dataset's own; the others are proper pairs (0x1|0x2, never 0x8), first and second mates and both strands in equal
    parts, TLEN +T or -T, CIGAR <T>M with T in [region_len, region_len + 80], start in [2, glen - T - 2], and a SEQ of n
    bases where n is short (1, 2, N-1, N, N+1, T-N-1, T-N, T-N+1, T-1), T itself, long (T+1, T+2, T+N, 2T, up to T+200)
    or absent (SEQ * with QUAL *).  N runs over the tests' -r values up to region_len.  SEQ is the reference slice with
    10 % substitutions; QUAL comes from QUAL_VALUES."""
    contigs, refs, fuzz = tl.fuzz_dataset(seed, n_reads, contig_lens=contig_lens, with_rg=with_rg)
    rng = np.random.default_rng(seed + 4242)
    ns = sorted({region_len, *(x for x in ROW_PASSES if x <= region_len)})
    recs = []
    for i in range(n_reads):
        if rng.random() < 1 / 3:
            recs.append(fuzz[i])
            continue
        t = int(rng.integers(region_len, region_len + 81))
        fit = [c for c in contigs if len(c[1]) >= t + 4]
        cname, ctext = fit[int(rng.integers(0, len(fit)))]
        s = int(rng.integers(2, len(ctext) - t - 2 + 1))
        n_of = int(ns[int(rng.integers(0, len(ns)))])
        u = rng.random()
        if u < 0.42:
            pool = [v for v in (1, 2, n_of - 1, n_of, n_of + 1, t - n_of - 1, t - n_of, t - n_of + 1, t - 1) if 1 <= v < t]
            n = pool[int(rng.integers(0, len(pool)))] if pool else t
        elif u < 0.52:
            n = t
        elif u < 0.94:
            n = (t + 1, t + 2, t + n_of, 2 * t, t + int(rng.integers(3, 201)))[int(rng.integers(0, 5))]
        else:
            n = 0
        mate, strand = CLASSES[i % 4]
        flag = 0x1 | 0x2 | mate | strand | (0x20 if rng.random() < 0.5 else 0)
        if n:
            seq = list(ctext[s:s + n].upper())
            seq += ["ACGT"[int(x)] for x in rng.integers(0, 4, size=n - len(seq))]     # SEQ may run past the contig
            for j in np.flatnonzero(rng.random(n) < 0.10):
                seq[j] = [b for b in "ACGT" if b != seq[j]][int(rng.integers(0, 3))]
            seq = "".join(seq)
            qual = "".join(chr(33 + QUAL_VALUES[int(x)]) for x in rng.integers(0, len(QUAL_VALUES), size=n))
        else:
            seq = qual = "*"
        tags = []
        if with_rg and rng.random() < 0.85:
            tags.append(("RG", "Z", "grpA" if rng.random() < 0.5 else "grpB"))
        recs.append(tl.Rec(qname=_name(rng, i), flag=flag, rname=cname, pos=s + 1, mapq=int(rng.integers(0, 61)), cigar=[(t, "M")],
                           tlen=t if rng.random() < 0.5 else -t, seq=seq, qual=qual, tags=tags))
    return contigs, refs, recs


def normalise(recs: list) -> list:
    """SEQ and QUAL of every governed record cut to |TLEN| bases, or padded on the right to |TLEN| with N (quality 40);
    every other record passes through unchanged"""
    out = []
    for r in recs:
        if not governed(r):
            out.append(r)
            continue
        t = abs(r.tlen)
        seq, qual = ("", "") if r.seq == "*" else (r.seq, r.qual)
        out.append(replace(r, seq=seq[:t].ljust(t, "N"), qual=qual[:t].ljust(t, "I")))
    return out


def reads_right_end(r: tl.Rec) -> bool:
    """does the one table a mate is added to take its window from the right end of SEQ as stored?  (The forward table
    reads the 5' end: the left of a forward-strand read, the right of a reverse-strand one; the reverse table the other.)"""
    return bool(r.flag & 0x40) == bool(r.flag & 0x10)


def anchor_on_l_seq(recs: list) -> list:
    """WRONG on purpose: the 3' end of SEQ as stored is taken from the end of SEQ, base T-1-i from SEQ[l_seq-1-i].  For
    the crafted records, which are added to one table each, as records the oracle can run on."""
    out = []
    for r, nr in zip(recs, normalise(recs)):
        if r.qname.startswith("d") and governed(r) and r.seq != "*" and reads_right_end(r):
            t, n = abs(r.tlen), len(r.seq)
            nr = replace(nr, seq="".join(r.seq[k - (t - n)] if 0 <= k - (t - n) < n else "N" for k in range(t)))
        out.append(nr)
    return out


def unblanked(recs: list) -> list:
    """WRONG on purpose: bases at or past l_seq are read from the nibbles that follow SEQ in the BAM record -- the pad
    nibble of an odd l_seq, then QUAL (past QUAL the model gives N).  The identity on records whose SEQ is long enough."""
    out = []
    for r, nr in zip(recs, normalise(recs)):
        if r.qname.startswith("d") and governed(r) and r.seq != "*" and len(r.seq) < abs(r.tlen):
            t, n = abs(r.tlen), len(r.seq)
            nib = [0] * (n & 1)
            for c in r.qual:
                nib += [(ord(c) - 33) >> 4, (ord(c) - 33) & 15]
            tail = "".join(tl.SEQ_CODES[x] for x in nib)[:t - n].ljust(t - n, "N")
            nr = replace(nr, seq=r.seq + tail)
        out.append(nr)
    return out


def record_offsets(refs, recs) -> list:
    """the byte offset of every record in the record block tl.raw_records builds"""
    idx = {n: i for i, (n, _) in enumerate(refs)}
    out, o = [], 0
    for r in recs:
        out.append(o)
        o += len(tl.bam_record(r, idx))
    return out

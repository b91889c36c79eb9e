"""The yardstick of pss-bam -n / -N / -V, shared by test_mismatch_host.py and test_gpu_mismatch.py.

The mismatch count m of a record (include/pssbam_hip.h, pssbam_engine_set_mismatches) restated in plain Python, the
reduced inputs the contract is written in -- RED(k), the input without the records whose m exceeds k, and the per-bin
subsets of the histogram identities -- and makers of hand-built records for the edge cases."""
from __future__ import annotations

import numpy as np

import pssbam_testlib as tl

ACGT = "ACGT"
TRANSITIONS = ({"A", "G"}, {"C", "T"})


def pss_length(rec: tl.Rec) -> int:
    """the length -l / -L compare: |TLEN| of a paired read, else the length of the SEQ text ('*' is one character)"""
    return abs(rec.tlen) if rec.flag & 1 else len(rec.seq)


def mismatches(rec: tl.Rec, contigs, tv_only: bool = False):
    """m of a record whose CIGAR is exactly <L>M on a contig of the FASTA, over the part of its span that lies inside
    the contig; None where m is not defined.  contigs: [(id, text)] as written (any case) or {id: text}."""
    ctg = contigs if isinstance(contigs, dict) else dict(contigs)
    L = pss_length(rec)
    if rec.cigar != [(L, "M")] or rec.rname not in ctg:
        return None
    g = ctg[rec.rname].upper()
    seq = "" if rec.seq == "*" else rec.seq.upper()
    s = rec.pos - 1
    m = 0
    for i in range(min(L, len(seq))):
        p = s + i
        if not 0 <= p < len(g):
            continue
        a, b = seq[i], g[p]
        if a in ACGT and b in ACGT and a != b and not (tv_only and {a, b} in TRANSITIONS):
            m += 1
    return m


REJECT_FLAGS = 0x4 | 0x100 | 0x200 | 0x400 | 0x800


def span_mismatches(rec: tl.Rec, contigs, tv_only: bool = False, candidates: bool = False):
    """the same count for the population the non-vacuity figures are taken over: a single-M record whose CIGAR length is
    its SEQ length, on a contig of the FASTA, with a POS -- paired or not, whatever its TLEN says; candidates: and none
    of the FLAG bits both tools reject.  None for every other record."""
    ctg = contigs if isinstance(contigs, dict) else dict(contigs)
    if rec.cigar != [(len(rec.seq), "M")] or rec.rname not in ctg or rec.pos < 1 or (candidates and rec.flag & REJECT_FLAGS):
        return None
    return mismatches(tl.Rec(**{**rec.__dict__, "flag": rec.flag & ~1}), ctg, tv_only)


def reduce_to(recs, contigs, k: int, tv_only: bool = False) -> list:
    """RED(k): the records without those whose m is defined and exceeds k"""
    ctg = dict(contigs)
    out = []
    for r in recs:
        m = mismatches(r, ctg, tv_only)
        if m is None or m <= k:
            out.append(r)
    return out


def split_by_bin(recs, contigs, M: int, tv_only: bool = False) -> list:
    """[bin 0, ..., bin M, bin M + 1]: the records whose min(m, M + 1) equals the bin (records without an m can never be
    added to a table and are in no bin)"""
    ctg = dict(contigs)
    bins: list = [[] for _ in range(M + 2)]
    for r in recs:
        m = mismatches(r, ctg, tv_only)
        if m is not None:
            bins[min(m, M + 1)].append(r)
    return bins


def bin_counts(recs, contigs, M: int, tv_only: bool = False) -> np.ndarray:
    return np.array([len(b) for b in split_by_bin(recs, contigs, M, tv_only)], dtype=np.int64)


def read_sam(path) -> tuple[list, list]:
    """(refs, recs) of a SAM text file: the eleven fixed fields, tags left out (no filter of the tools reads them here)"""
    refs, recs = [], []
    for ln in open(path):
        if ln.startswith("@"):
            if ln.startswith("@SQ"):
                f = dict(x.split(":", 1) for x in ln.rstrip("\n").split("\t")[1:])
                refs.append((f["SN"], int(f["LN"])))
            continue
        f = ln.rstrip("\n").split("\t")
        cigar = []
        if f[5] != "*":
            n = ""
            for ch in f[5]:
                if ch.isdigit():
                    n += ch
                else:
                    cigar.append((int(n), ch))
                    n = ""
        recs.append(tl.Rec(qname=f[0], flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=cigar, rnext=f[6],
                           pnext=int(f[7]), tlen=int(f[8]), seq=f[9], qual=f[10]))
    return refs, recs


def reduce_sam_text(text: str, contigs, k: int, tv_only: bool = False) -> str:
    """RED(k) on SAM text: header lines and every kept record line pass through byte for byte"""
    ctg = dict(contigs)
    out = []
    for ln in text.splitlines(keepends=True):
        if not ln.startswith("@"):
            f = ln.rstrip("\n").split("\t")
            cigar = [(int(f[5][:-1]), "M")] if f[5][:-1].isdigit() and f[5].endswith("M") else [(0, "?")]
            r = tl.Rec(qname=f[0], flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=cigar, tlen=int(f[8]), seq=f[9], qual=f[10])
            m = mismatches(r, ctg, tv_only)
            if m is not None and m > k:
                continue
        out.append(ln)
    return "".join(out)


# ---- hand-built records ----------------------------------------------------------------------------------------------

OTHER = {"A": "C", "C": "A", "G": "T", "T": "G"}      # a transversion partner of every base


def clean_contig(n: int, seed: int = 11) -> str:
    """n bases of upper-case A/C/G/T"""
    rng = np.random.default_rng(seed)
    return "".join(ACGT[int(x)] for x in rng.integers(0, 4, size=n))


def read_on(ctg_text: str, s: int, L: int, subs=None, name: str = "r", flag: int = 0, rname: str = "c", tlen: int = 0,
            seq_len: int | None = None, mapq: int = 30) -> tl.Rec:
    """the <L>M record at 0-based start s that copies the (upper-cased) contig except where subs = {read position: base}
    says otherwise; seq_len: SEQ shorter or longer than L (a paired record, whose L is |TLEN|)"""
    n = L if seq_len is None else seq_len
    seq = list(ctg_text[s:s + n].upper().ljust(n, "A"))
    for i, b in (subs or {}).items():
        seq[i] = b
    return tl.Rec(qname=name, flag=flag, rname=rname, pos=s + 1, mapq=mapq, cigar=[(L, "M")], tlen=tlen, seq="".join(seq), qual="I" * n)


def with_mismatches(ctg_text: str, s: int, L: int, positions, **kw) -> tl.Rec:
    """read_on with a transversion at each of the given read positions (the contig must hold A/C/G/T there)"""
    return read_on(ctg_text, s, L, {i: OTHER[ctg_text[s + i].upper()] for i in positions}, **kw)

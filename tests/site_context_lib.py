"""The yardstick of pss-bam -X cpg, shared by test_site_context_host.py and test_gpu_site_context.py.

Position p of a contig g (upper-cased, as the tools fold it) is in CpG context when g[p] is a C followed by a G or a G
preceded by a C; a neighbour outside the contig counts as "no".  Nothing in the reference looks at the content of SEQ
except add_fwd_counts / add_rev_counts, and they skip a read base that is not A/C/G/T, so

    IN  == the tool without -X on the same records with SEQ base k set to N wherever POS-1+k is NOT in context,
    OUT == the same with the complementary mask.

mask_recs / mask_sam_text build those inputs; direct_counts is an independent count that skips the positions
instead, against which the masker is checked once (on the CPU oracle)."""
from __future__ import annotations

from dataclasses import replace

import numpy as np

import pssbam_testlib as tl


def in_cpg(contig: str, p: int) -> bool:
    """contig: upper-case bases; p: 0-based position (outside the contig: False)"""
    if not 0 <= p < len(contig):
        return False
    c = contig[p]
    return (c == "C" and p + 1 < len(contig) and contig[p + 1] == "G") or (c == "G" and p >= 1 and contig[p - 1] == "C")


def cpg_flags(contig: str) -> np.ndarray:
    """in_cpg of every position at once"""
    a = np.frombuffer(contig.upper().encode(), dtype=np.uint8)
    f = np.zeros(a.size, dtype=bool)
    if a.size > 1:
        cg = (a[:-1] == ord("C")) & (a[1:] == ord("G"))
        f[:-1] |= cg
        f[1:] |= cg
    return f


def mask_seq(seq: str, flags, s: int, keep_in: bool) -> str:
    """SEQ with base k set to N where contig position s + k is not of the kept kind (or outside the contig)"""
    if seq == "*":
        return seq
    n = len(flags)
    return "".join(b if 0 <= s + k < n and bool(flags[s + k]) == keep_in else "N" for k, b in enumerate(seq))


def mask_recs(contigs, recs: list, keep_in: bool) -> list:
    """records on a contig the genome lacks are tallied by nobody and stay as they are"""
    flags = {cid: cpg_flags(seq) for cid, seq in contigs}
    return [replace(r, seq=mask_seq(r.seq, flags[r.rname], r.pos - 1, keep_in)) if r.rname in flags else r for r in recs]


def mask_sam_text(text: str, contigs, keep_in: bool) -> str:
    """the same on SAM text (header lines pass through)"""
    flags = {cid: cpg_flags(seq) for cid, seq in contigs}
    out = []
    for ln in text.splitlines(keepends=True):
        if not ln.startswith("@"):
            f = ln.rstrip("\n").split("\t")
            if f[2] in flags:
                f[9] = mask_seq(f[9], flags[f[2]], int(f[3]) - 1, keep_in)
            ln = "\t".join(f) + "\n"
        out.append(ln)
    return "".join(out)


def read_fasta(path) -> list:
    """[(id, bases)] of a FASTA file, the id up to the first blank"""
    out = []
    for ln in open(path):
        if ln.startswith(">"):
            out.append([ln[1:].split()[0], []])
        elif ln.strip():
            out[-1][1].append(ln.strip())
    return [(cid, "".join(parts)) for cid, parts in out]


_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
FL_REJECT = 0x4 | 0x100 | 0x200 | 0x400 | 0x800


def direct_counts(contigs, recs, o: tl.PssOpts, keep_in):
    """pss-bam's tables (fwd, rev) counted straight from the records, leaving out every interior position whose
    reference position is not of the kept kind (keep_in None: every position counts).  Restates process_aln's filters;
    -U / -D as sets of characters (the tests use sets without the terminator's corner case)."""
    genome = {cid: seq.upper() for cid, seq in contigs}
    n = o.region_len
    fwd = np.zeros((n + 2, 16), dtype=np.uint64)
    rev = np.zeros_like(fwd)
    for r in recs:
        if len(r.seq) != len(r.qual):
            continue                                    # line2saml: skipped
        ref = genome.get(r.rname)
        if ref is None:
            continue
        paired = bool(r.flag & 1)
        L = abs(r.tlen) if paired else len(r.seq)
        s = r.pos - 1
        if s - 2 < 0 or s + L + 2 > len(ref):
            continue
        if r.mapq < o.min_mq or not (o.min_read_len <= L <= o.max_read_len and L >= n):
            continue
        if r.cigar_str() != f"{L}M" or (r.flag & FL_REJECT) or (o.merged_only and paired):
            continue
        is_rev = bool(r.flag & 0x10)

        def put(tab, row, rd, rf):                      # genome-orientation bases; reverse-strand reads complement both
            if is_rev:
                rd, rf = _COMP.get(rd, rd), _COMP.get(rf, rf)
            if rd in _CODE and rf in _CODE:
                tab[row, 4 * _CODE[rd] + _CODE[rf]] += 1

        def end(tab, left):
            c1, c0 = (ref[s - 1], ref[s - 2]) if left else (ref[s + L], ref[s + L + 1])
            put(tab, 0, c0, c0)
            put(tab, 1, c1, c1)
            for i in range(n):
                k = i if left else L - 1 - i
                if k >= len(r.seq) or (keep_in is not None and in_cpg(ref, s + k) != keep_in):
                    continue
                put(tab, i + 2, r.seq[k].upper(), ref[s + k])

        first_l, first_r = ref[s - 1], ref[s + L]      # first context base on either side
        up = _COMP.get(first_r, first_r) if is_rev else first_l
        dn = _COMP.get(first_l, first_l) if is_rev else first_r
        up_ok, dn_ok = up in o.up_ctx, dn in o.down_ctx
        do_fwd = do_rev = False
        if not paired:
            do_fwd = do_rev = up_ok and dn_ok
        elif (r.flag & 0x2) and not (r.flag & 0x8):
            if (r.flag & 0x40) and up_ok:
                do_fwd = True
            elif (r.flag & 0x80) and dn_ok:
                do_rev = True
        # forward-strand read: fwd table <- left end, rev table <- right end; reverse-strand read: the other way round
        if do_fwd:
            end(fwd, not is_rev)
        if do_rev:
            end(rev, is_rev)
    return fwd, rev

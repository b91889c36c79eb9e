"""The yardstick of pss-bam -Q, shared by test_base_quality_host.py and test_gpu_base_quality.py.

`pss-bam -Q q` on a file == the tool without -Q on the same file with every SEQ base whose quality is below q
replaced by N (a read base that is not A/C/G/T adds nothing; nothing else looks at the content of SEQ).  mask_recs /
write_masked_sam build that second file; direct_pss_counts is an independent count that skips the low-quality
positions instead, against which the masker is checked once (on the CPU oracle)."""
from __future__ import annotations

from dataclasses import replace
from pathlib import Path

import numpy as np

import pssbam_testlib as tl


def mask_seq(seq: str, qual: str, q: int) -> str:
    """SEQ with every base whose Phred quality (QUAL character - 33) is below q set to N; '*' SEQ or QUAL: untouched"""
    if seq == "*" or qual == "*" or len(seq) != len(qual):
        return seq
    return "".join("N" if ord(c) - 33 < q else b for b, c in zip(seq, qual))


def mask_recs(recs: list, q: int) -> list:
    return [replace(r, seq=mask_seq(r.seq, r.qual, q)) for r in recs]


def write_masked_sam(path: Path, refs, recs, q: int) -> None:
    tl.write_sam(path, refs, mask_recs(recs, q))


def mask_sam_text(text: str, q: int) -> str:
    """the same on SAM text (header lines pass through)"""
    out = []
    for ln in text.splitlines(keepends=True):
        if ln.startswith("@"):
            out.append(ln)
            continue
        f = ln.rstrip("\n").split("\t")
        f[9] = mask_seq(f[9], f[10], q)
        out.append("\t".join(f) + "\n")
    return "".join(out)


_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
FL_REJECT = 0x4 | 0x100 | 0x200 | 0x400 | 0x800


def direct_pss_counts(contigs, recs, o: tl.PssOpts, q: int):
    """pss-bam's tables (fwd, rev) counted straight from the records, leaving out every interior position whose read
    base has a quality below q.  Restates process_aln's filters; -U / -D as sets of characters (the tests use sets
    without the terminator's corner case)."""
    genome = {cid: seq.upper() for cid, seq in contigs}
    n = o.region_len
    fwd = np.zeros((n + 2, 16), dtype=np.uint64)
    rev = np.zeros_like(fwd)

    def comp(c):
        return _COMP.get(c, c)

    for r in recs:
        if len(r.seq) != len(r.qual):
            continue                                    # line2saml: skipped
        ref = genome.get(r.rname)
        if ref is None:
            continue
        paired = bool(r.flag & 1)
        L = abs(r.tlen) if paired else len(r.seq)
        s = r.pos - 1
        if s - 2 < 0 or s + L - 1 + 2 > len(ref) - 1:
            continue
        if r.mapq < o.min_mq or not (o.min_read_len <= L <= o.max_read_len and L >= n):
            continue
        if r.cigar_str() != f"{L}M" or (r.flag & FL_REJECT) or (o.merged_only and paired):
            continue
        is_rev = bool(r.flag & 0x10)

        def g(j):                                       # the window s-2 .. s+L+1 in read orientation
            return comp(ref[s - 2 + (L + 3 - j)]) if is_rev else ref[s - 2 + j]

        def rd(i):                                      # read base i in read orientation, None when masked / absent
            k = L - 1 - i if is_rev else i
            if not 0 <= k < len(r.seq):
                return None
            if r.qual != "*" and ord(r.qual[k]) - 33 < q:
                return None
            c = r.seq[k].upper()
            return comp(c) if is_rev else c

        up_ok, dn_ok = g(1) in o.up_ctx, g(L + 2) in o.down_ctx

        def ctx(tab, first, second):
            if second in _CODE:
                tab[0, 5 * _CODE[second]] += 1
            if first in _CODE:
                tab[1, 5 * _CODE[first]] += 1

        def tally_fwd():
            ctx(fwd, g(1), g(0))
            for i in range(n):
                a, b = rd(i), g(2 + i)
                if a in _CODE and b in _CODE:
                    fwd[i + 2, 4 * _CODE[a] + _CODE[b]] += 1

        def tally_rev():
            ctx(rev, g(L + 2), g(L + 3))
            for i in range(n):
                a, b = rd(L - 1 - i), g(L + 1 - i)
                if a in _CODE and b in _CODE:
                    rev[i + 2, 4 * _CODE[a] + _CODE[b]] += 1

        if not paired:
            if up_ok and dn_ok:
                tally_fwd()
                tally_rev()
        elif (r.flag & 0x2) and not (r.flag & 0x8):
            if (r.flag & 0x40) and up_ok:
                tally_fwd()
            elif (r.flag & 0x80) and dn_ok:
                tally_rev()
    return fwd, rev

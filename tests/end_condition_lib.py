"""The yardstick of pss-bam -E, shared by test_end_condition_host.py and test_gpu_end_condition.py.

For a record let o / g be the read and reference bases as process_aln pairs them: upper case, both
reverse-complemented for a FLAG 0x10 read.  cell(r, f) = 4 * code(r) + code(f) with A 0, C 1, G 2, T 3; a pair with a
member that is not A/C/G/T has no cell, and neither has a read base whose quality is below the minimum base quality.
An unpaired record is 5'-marked when cell(o[i], g[i]) == cell5 for some i < depth, and 3'-marked when
cell(o[L-1-i], g[L-1-i]) == cell3 for some i < depth.  Then

    COND.fwd == the forward table of the tool without -E on the input reduced to the unpaired 3'-marked records,
    COND.rev == the reverse table on the input reduced to the unpaired 5'-marked records,
    reads    == PSS_OK of the tool on the unpaired records / the 5'-marked / the 3'-marked / the both-marked ones.

marks() is written from that definition alone; reduce_recs / reduce_sam_text build the reduced inputs, and
direct_counts is an independent count against which the reduction is checked once (on the CPU oracle)."""
from __future__ import annotations

from dataclasses import replace

import numpy as np

import pssbam_testlib as tl
import site_context_lib as sc

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
PRESETS = {"ss": (13, 13), "ds": (13, 2)}


def cell_of(r: str, f: str):
    return 4 * _CODE[r] + _CODE[f] if r in _CODE and f in _CODE else None


def _marks(genome: dict, rname: str, flag: int, pos: int, seq: str, qual: str, depth: int, cell5: int, cell3: int, min_bq: int):
    if flag & 1 or seq == "*":
        return False, False
    ref = genome.get(rname)
    if ref is None:
        return False, False
    L, s = len(seq), pos - 1
    if s < 0 or s + L > len(ref) or L < depth:
        return False, False                             # such a record is tallied by nobody
    o, g = seq.upper(), ref[s:s + L]
    q = [ord(c) - 33 for c in qual] if qual != "*" and len(qual) == L else [255] * L
    if flag & 0x10:
        o = "".join(_COMP.get(c, "N") for c in reversed(o))
        g = "".join(_COMP.get(c, "N") for c in reversed(g))
        q = q[::-1]
    cells = [None if q[k] < min_bq else cell_of(o[k], g[k]) for k in range(L)]
    m5 = any(cells[i] == cell5 for i in range(depth))
    m3 = any(cells[L - 1 - i] == cell3 for i in range(depth))
    return m5, m3


def genome_of(contigs) -> dict:
    return {cid: seq.upper() for cid, seq in contigs}


def marks(contigs, rec: tl.Rec, depth: int, cell5: int, cell3: int, min_bq: int = 0):
    """(5'-marked, 3'-marked) of one record; contigs: [(id, bases)] or the dict genome_of() makes of them"""
    genome = contigs if isinstance(contigs, dict) else genome_of(contigs)
    return _marks(genome, rec.rname, rec.flag, rec.pos, rec.seq, rec.qual, depth, cell5, cell3, min_bq)


def keep(m5: bool, m3: bool, which: str) -> bool:
    return {"5": m5, "3": m3, "both": m5 and m3}[which]


def reduce_recs(contigs, recs: list, depth: int, cell5: int, cell3: int, which: str, min_bq: int = 0) -> list:
    """the unpaired records that are 5'-marked (which = "5"), 3'-marked ("3") or both ("both"); "unpaired": every
    unpaired record"""
    genome = genome_of(contigs)
    if which == "unpaired":
        return [r for r in recs if not r.flag & 1]
    return [r for r in recs if keep(*marks(genome, r, depth, cell5, cell3, min_bq), which)]


def reduce_sam_text(text: str, contigs, depth: int, cell5: int, cell3: int, which: str, min_bq: int = 0) -> str:
    """the same on SAM text (header lines pass through)"""
    genome = genome_of(contigs)
    out = []
    for ln in text.splitlines(keepends=True):
        if not ln.startswith("@"):
            f = ln.rstrip("\n").split("\t")
            flag = int(f[1])
            if which == "unpaired":
                if flag & 1:
                    continue
            elif not keep(*_marks(genome, f[2], flag, int(f[3]), f[9], f[10], depth, cell5, cell3, min_bq), which):
                continue
        out.append(ln)
    return "".join(out)


def plant_damage(contigs, recs: list, rng: np.random.Generator, rate: float, reach: int = 3) -> list:
    """Terminal deamination on copies of the records: within `reach` bases of either alignment end a read base on a
    reference C becomes T and one on a reference G becomes A (genome orientation; on one strand or the other these are
    the C->T and G->A of both presets at both ends), with a probability that falls off inward as rate / (1 + distance)"""
    genome = genome_of(contigs)
    out = []
    for r in recs:
        ref = genome.get(r.rname)
        s, L = r.pos - 1, len(r.seq)
        if ref is None or r.seq == "*" or s < 0 or s + L > len(ref):
            out.append(r)
            continue
        seq = list(r.seq)
        for i in range(min(reach, L)):
            for k in (i, L - 1 - i):
                if rng.random() < rate / (1 + i):
                    seq[k] = {"C": "T", "G": "A"}.get(ref[s + k], seq[k])
        out.append(replace(r, seq="".join(seq)))
    return out


def expected(oracle, g, tmp, refs, contigs, recs, o: tl.PssOpts, depth: int, cell5: int, cell3: int, min_bq: int = 0, mask=None):
    """(COND.fwd, COND.rev, reads[4]) from the oracle on the reduced inputs.  `mask` (records -> records) is applied to
    every reduced input before the oracle sees it: the N-masking that stands for -Q."""
    reads = np.zeros(4, dtype=np.uint64)
    tabs = {}
    for k, which in enumerate(("unpaired", "5", "3", "both")):
        part = reduce_recs(contigs, recs, depth, cell5, cell3, which, min_bq)
        sam = tmp / f"red_{which}.sam"
        tl.write_sam(sam, refs, mask(part) if mask else part)
        fwd, rev, st = oracle.pss(g, sam, o)
        reads[k] = st[tl.ST_OK]
        tabs[which] = (fwd, rev)
    return tabs["3"][0], tabs["5"][1], reads


def direct_counts(contigs, recs, o: tl.PssOpts, depth: int, cell5: int, cell3: int):
    """(COND.fwd, COND.rev, reads[4]) counted straight from the records: site_context_lib.direct_counts (every position
    counts) over one record at a time decides "added to the tables" and gives the record's contribution"""
    n = o.region_len
    cf, cr = np.zeros((n + 2, 16), dtype=np.uint64), np.zeros((n + 2, 16), dtype=np.uint64)
    reads = np.zeros(4, dtype=np.uint64)
    genome = genome_of(contigs)
    for r in recs:
        if r.flag & 1:
            continue
        fwd, rev = sc.direct_counts(contigs, [r], o, None)
        if not (fwd.any() or rev.any()):
            continue
        m5, m3 = marks(genome, r, depth, cell5, cell3)
        reads += np.array([1, m5, m3, m5 and m3], dtype=np.uint64)
        if m3:
            cf += fwd
        if m5:
            cr += rev
    return cf, cr, reads

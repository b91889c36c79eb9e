"""The yardstick of pss-bam -W, shared by test_interior_host.py, test_gpu_interior.py and tests/golden/make_interior_golden.py.

The interior table (include/pssbam_hip.h, pssbam_engine_set_interior) restated in plain Python: which records are added to
a table (the filters of the reference's process_aln, as oracle/pss_oracle.c restates them), and what their interior
positions count.  Builders of hand-built records come from mismatch_lib; the golden reducer sums the rows of the
reference's per-length runs."""
from __future__ import annotations

import numpy as np

import mismatch_lib as ml
import pssbam_testlib as tl

ACGT = "ACGT"
REJECT_FLAGS = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}

read_on, with_mismatches, clean_contig, pss_length, OTHER = ml.read_on, ml.with_mismatches, ml.clean_contig, ml.pss_length, ml.OTHER


def tables_entered(rec: tl.Rec, ctg: dict, o: tl.PssOpts) -> tuple[bool, bool]:
    """(forward, reverse): the tables a record is added to -- every record filter of the run, then the mate rules and
    -U / -D (oracle/pss_oracle.c: orc_pss_process; a line whose SEQ and QUAL texts differ in length is dropped by the parser)"""
    if len(rec.seq) != len(rec.qual) or rec.rname not in ctg:
        return False, False
    g = ctg[rec.rname]
    L = pss_length(rec)
    s = rec.pos - 1
    if s - 2 < 0 or s + L - 1 + 2 > len(g) - 1:
        return False, False
    if rec.mapq < o.min_mq or not (o.min_read_len <= L <= o.max_read_len and L >= o.region_len):
        return False, False
    if rec.cigar != [(L, "M")] or rec.flag & REJECT_FLAGS or (o.merged_only and rec.flag & 1):
        return False, False
    left1, right1 = g[s - 1].upper(), g[s + L].upper()
    rev = bool(rec.flag & 0x10)
    up1 = COMP.get(right1, right1) if rev else left1
    dn1 = COMP.get(left1, left1) if rev else right1
    up_ok, dn_ok = up1 in o.up_ctx, dn1 in o.down_ctx
    if not rec.flag & 1:
        return (up_ok and dn_ok,) * 2
    if rec.flag & 0x2 and not rec.flag & 0x8:
        if rec.flag & 0x40 and up_ok:
            return True, False
        if rec.flag & 0x80 and dn_ok:
            return False, True
    return False, False


def record_interior(rec: tl.Rec, ctg: dict, d: int, min_bq: int = 0):
    """(bins[16], has_interior) of one record that is added to a table: I = {i : d <= i, i + d < L, i < l_seq}"""
    bins = np.zeros(16, dtype=np.uint64)
    g = ctg[rec.rname]
    L = pss_length(rec)
    seq = "" if rec.seq == "*" else rec.seq.upper()
    qual = None if rec.qual == "*" else rec.qual       # absent qualities mask nothing
    s = rec.pos - 1
    hi = min(L - d, len(seq))
    for i in range(d, hi):
        a, b = seq[i], g[s + i].upper()
        if a not in ACGT or b not in ACGT:
            continue
        if min_bq and qual is not None and ord(qual[i]) - 33 < min_bq:
            continue
        cell = 4 * ACGT.index(a) + ACGT.index(b)
        bins[15 - cell if rec.flag & 0x10 else cell] += 1
    return bins, hi > d


def interior(recs, contigs, d: int, o: tl.PssOpts | None = None, min_bq: int = 0):
    """(table u64[16], reads, tallied): the interior table of a run over recs, the records whose interior is not empty, and
    the records that are added to a table at all.  contigs: [(id, text)] or {id: text}."""
    ctg = contigs if isinstance(contigs, dict) else dict(contigs)
    o = o or tl.PssOpts()
    table, reads, tallied = np.zeros(16, dtype=np.uint64), 0, 0
    for r in recs:
        if not any(tables_entered(r, ctg, o)):
            continue
        tallied += 1
        bins, some = record_interior(r, ctg, d, min_bq)
        table += bins
        reads += int(some)
    return table, reads, tallied


def lane_cut(d: int, L: int, l_seq: int | None = None) -> int:
    """where the tiled kernel cuts the interior [d, min(L - d, l_seq)) between the two lanes of a read's pair"""
    hi = min(L - d, L if l_seq is None else l_seq)
    lo8 = d & ~7
    return min(hi, lo8 + ((((hi - lo8) >> 1) + 7) & ~7)) if hi > d else d


# ---- the golden reducer ----------------------------------------------------------------------------------------------

def rows_sum(table: np.ndarray, d: int, x: int) -> np.ndarray:
    """rows d .. x-d-1 (positions; the two context rows lie in front of them) of a table of region_len x - d, summed"""
    assert table.shape == (x - d + 2, 16)
    return table[2 + d:2 + x - d].sum(axis=0, dtype=np.uint64)


def split_sam(recs):
    """(unpaired, paired)"""
    return [r for r in recs if not r.flag & 1], [r for r in recs if r.flag & 1]


def reduce_runs(d: int, unpaired_runs: dict, paired_runs: dict) -> np.ndarray:
    """the interior table from per-length runs `-l x -L x -r x-d`: {x: (fwd, rev)} of the unpaired and of the paired records.
    Unpaired reads appear whole in the forward rows; a read 1 appears in the forward rows only, a read 2 in the reverse
    rows only (row i from the 3' end is read position x-1-i: the same set of positions)."""
    table = np.zeros(16, dtype=np.uint64)
    for x, (fwd, _) in unpaired_runs.items():
        table += rows_sum(fwd, d, x)
    for x, (fwd, rev) in paired_runs.items():
        table += rows_sum(fwd, d, x) + rows_sum(rev, d, x)
    return table


def golden_text(d: int, table, reads: int, tallied: int) -> str:
    return (f"margin\t{d}\ntable\t" + "\t".join(str(int(v)) for v in table) + f"\nreads\t{reads}\nbases\t{int(np.sum(table))}\n"
            f"tallied\t{tallied}\n")


def parse_golden(text: str) -> dict:
    f = dict(ln.split("\t", 1) for ln in text.splitlines())
    return {"margin": int(f["margin"]), "table": np.array([int(v) for v in f["table"].split("\t")], dtype=np.uint64),
            "reads": int(f["reads"]), "bases": int(f["bases"]), "tallied": int(f["tallied"])}


def parse_interior_file(text: str) -> dict:
    """<prefix>.pss.interior.txt -> {"comment", "label", "table", "rates" (text fields), "reads", "bases"}"""
    lines = text.splitlines()
    assert lines[0].startswith("# ") and lines[1].startswith("# FASTA: ") and lines[2].startswith("# BAM: ")
    assert lines[3] == "### POS AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT" and lines[5] == "### POS AC AG AT CA CG CT GA GC GT TA TC TG"
    counts, rates = lines[4].split("\t"), lines[6].split("\t")
    assert counts[-1] == "" and rates[-1] == "" and len(counts) == 18 and len(rates) == 14 and counts[0] == rates[0]
    assert lines[7].startswith("reads\t") and lines[8].startswith("bases\t") and len(lines) == 9
    return {"comment": lines[0], "label": int(counts[0]), "table": np.array([int(v) for v in counts[1:17]], dtype=np.uint64),
            "rates": rates[1:13], "reads": int(lines[7].split("\t")[1]), "bases": int(lines[8].split("\t")[1])}


def expected_rates(table) -> list[str]:
    """the twelve rates as the rates file prints them (find_sub_rates' rule: all zero when a reference column is empty)"""
    t = [int(v) for v in table]
    col = [t[r] + t[4 + r] + t[8 + r] + t[12 + r] for r in range(4)]
    off = [c for c in range(16) if c // 4 != c % 4]
    return ["%.5e" % (0.0 if 0 in col else t[c] / col[c & 3]) for c in off]

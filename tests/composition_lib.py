"""The yardstick of pss-bam -P, shared by test_composition_host.py, test_gpu_composition.py and
tests/golden/make_composition_golden.py.

The composition table (include/pssbam_hip.h, pssbam_engine_set_composition) restated in plain Python: which records are added
to which table comes from interior_lib.tables_entered; what their ends count is the definition, position by position.  The
builders of the all-A and the shifted records turn the table's rows into rows the unmodified reference prints (the three
ties of the header text), and the parser reads <prefix>.pss.composition.txt back."""
from __future__ import annotations

from dataclasses import replace

import numpy as np

import interior_lib as il
import pssbam_testlib as tl

ACGT = "ACGT"
DIAG = (0, 5, 10, 15)      # the cells AA CC GG TT of a counts row: a context row holds its reference base there


def cls(x: str) -> int:
    """0 1 2 3 for A C G T, 4 for anything else (x after the case folding)"""
    return ACGT.index(x) if x in ACGT else 4


def comp(c: int) -> int:
    return 3 - c if c < 4 else 4


def record_composition(rec: tl.Rec, g: str, w: int, fwd: bool, rev_table: bool):
    """(c5, c3) of one record: arrays (2w, 5); g = the record's contig, folded to upper case"""
    c5, c3 = np.zeros((2 * w, 5), dtype=np.uint64), np.zeros((2 * w, 5), dtype=np.uint64)
    L, s, rev = il.pss_length(rec), rec.pos - 1, bool(rec.flag & 0x10)
    for block, on, left in ((c5, fwd, not rev), (c3, rev_table, rev)):
        if not on:
            continue
        for j in range(-w, w):
            if j >= 0 and j >= L:
                continue
            p = s + j if left else s + L - 1 - j
            if not 0 <= p < len(g):
                continue
            c = cls(g[p])
            block[j + w, comp(c) if rev else c] += 1
    return c5, c3


def composition(recs, contigs, w: int, o: tl.PssOpts | None = None):
    """(c5, c3, n_fwd, n_rev): the two blocks of a run over recs and the number of records added to the forward / reverse
    table.  contigs: [(id, text)] or {id: text}."""
    ctg = contigs if isinstance(contigs, dict) else dict(contigs)
    up = {k: v.upper() for k, v in ctg.items()}
    o = o or tl.PssOpts()
    c5, c3 = np.zeros((2 * w, 5), dtype=np.uint64), np.zeros((2 * w, 5), dtype=np.uint64)
    n_fwd = n_rev = 0
    for r in recs:
        f, v = il.tables_entered(r, ctg, o)
        if not (f or v):
            continue
        a, b = record_composition(r, up[r.rname], w, f, v)
        c5 += a
        c3 += b
        n_fwd += int(f)
        n_rev += int(v)
    return c5, c3, n_fwd, n_rev


def positions_exist(recs, contigs, w: int, o: tl.PssOpts | None = None):
    """(n5, n3): arrays (2w,), how many of the records added to the forward / reverse table have a position at offset j + w --
    what every row of the two blocks must sum to"""
    c5, c3, _, _ = composition(recs, contigs, w, o)
    return c5.sum(axis=1), c3.sum(axis=1)


# ---- the ties to the reference's own rows ------------------------------------------------------------------------------

def context_rows(fwd: np.ndarray, rev: np.ndarray) -> dict:
    """tie 1: {("c5", -1): [A, C, G, T], ("c5", -2): ..., ("c3", -1): ..., ("c3", -2): ...} from a run's tables (in-memory row order:
    row 0 = the second context base, row 1 = the first)"""
    return {(b, -k): [int(t[2 - k, c]) for c in DIAG] for b, t in (("c5", fwd), ("c3", rev)) for k in (1, 2)}


def all_a(recs):
    """tie 2: every SEQ replaced by A x l_seq.  QUAL stays as it is and so matches the new SEQ exactly where it matched the old
    one: a record the parser drops (QUAL absent, or of another length) is dropped before and after.  Records without a SEQ stay
    as they are."""
    return [r if r.seq == "*" else replace(r, seq="A" * len(r.seq)) for r in recs]


def inside_rows(fwd: np.ndarray, rev: np.ndarray, n: int) -> dict:
    """tie 2: {("c5", j): [A, C, G, T]} for j < n: the column sums over the read bases of position row j"""
    return {(b, j): [int(t[2 + j, x] + t[2 + j, 4 + x] + t[2 + j, 8 + x] + t[2 + j, 12 + x]) for x in range(4)]
            for b, t in (("c5", fwd), ("c3", rev)) for j in range(n)}


def far_from_edges(recs, contigs, w: int, min_len: int):
    """tie 3: the unpaired <L>M records at least w bases from both contig edges and at least min_len long"""
    ctg = contigs if isinstance(contigs, dict) else dict(contigs)
    out = []
    for r in recs:
        if r.flag & 1 or r.rname not in ctg or r.seq == "*" or r.cigar != [(len(r.seq), "M")] or len(r.seq) < min_len:
            continue
        s, L = r.pos - 1, len(r.seq)
        if s >= w and s + L + w <= len(ctg[r.rname]):
            out.append(r)
    return out


def shifted(recs, j: int, block: str):
    """tie 3: the records whose context row 2 is the original's outside row j (j >= 3).  For the 5' block a forward-strand record
    grows by j - 2 bases at its left side (POS moves), a reverse-strand record at its right side; for the 3' block the other
    way round.  The new bases are A, QUAL to match."""
    k = j - 2
    out = []
    for r in recs:
        L = len(r.seq)
        left = (block == "c5") != bool(r.flag & 0x10)
        if left:
            out.append(replace(r, pos=r.pos - k, seq="A" * k + r.seq, qual="I" * k + r.qual, cigar=[(L + k, "M")]))
        else:
            out.append(replace(r, seq=r.seq + "A" * k, qual=r.qual + "I" * k, cigar=[(L + k, "M")]))
    return out


def fasta_letters(contigs) -> str:
    """every letter of the contigs after the case folding, A C G T first: an -U / -D set that rejects nothing"""
    seen = set("".join(t for _, t in (contigs.items() if isinstance(contigs, dict) else contigs)).upper())
    return ACGT + "".join(sorted(seen - set(ACGT)))


# ---- the golden file: "<tie>\t<block>\t<offset>\t<A>\t<C>\t<G>\t<T>" -------------------------------------------------------

def golden_text(w: int, ties: dict) -> str:
    out = [f"width\t{w}\n"]
    for tie in sorted(ties):
        for (block, j), v in sorted(ties[tie].items()):
            out.append(f"{tie}\t{block}\t{j}\t" + "\t".join(str(int(x)) for x in v) + "\n")
    return "".join(out)


def parse_golden(text: str):
    """(w, {tie: {(block, offset): [A, C, G, T]}})"""
    lines = text.splitlines()
    assert lines[0].startswith("width\t")
    ties: dict = {}
    for ln in lines[1:]:
        tie, block, j, *v = ln.split("\t")
        ties.setdefault(tie, {})[(block, int(j))] = [int(x) for x in v]
    return int(lines[0].split("\t")[1]), ties


# ---- the composition file --------------------------------------------------------------------------------------------

def fractions(row) -> list[str]:
    """the four fractions of a row as the file prints them"""
    n = sum(int(x) for x in row[:4])
    return ["%.5e" % (int(x) / n if n else 0.0) for x in row[:4]]


def file_text(fasta: str, bam: str, w: int, c5, c3) -> str:
    """what pss_write_composition writes"""
    def row(label, r):
        return f"{label}\t" + "".join(f"{int(x)}\t" for x in r) + "".join(f"{x}\t" for x in fractions(r)) + "\n"
    out = [f"# reference base composition {w} bases on either side of the ends of the tallied reads, in the read's orientation"
           " (negative: outside the read)\n", f"# FASTA: {fasta}\n# BAM: {bam}\n", "### POS A C G T other fA fC fG fT\n",
           "### Forward read base composition around the 5' end\n"]
    out += [row(j, c5[j + w]) for j in range(-w, w)]
    out.append("\n\n### Reverse read base composition around the 3' end\n")
    out += [row(j, c3[j + w]) for j in range(w - 1, -1, -1)]
    out += [row(j, c3[w - j]) for j in range(1, w + 1)]
    return "".join(out)


def parse_composition_file(text: str):
    """<prefix>.pss.composition.txt -> (w, c5, c3, fractions5, fractions3): counts as (2w, 5) arrays, fractions as text fields"""
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0].startswith("# ") and lines[1].startswith("# FASTA: ") and lines[2].startswith("# BAM: ")
    assert lines[3] == "### POS A C G T other fA fC fG fT" and lines[4].startswith("### Forward")
    body = lines[5:-1]
    w = (len(body) - 3) // 4
    assert len(body) == 4 * w + 3 and body[2 * w] == "" and body[2 * w + 1] == "" and body[2 * w + 2].startswith("### Reverse")
    c5, c3 = np.zeros((2 * w, 5), dtype=np.uint64), np.zeros((2 * w, 5), dtype=np.uint64)
    f5, f3 = [None] * (2 * w), [None] * (2 * w)

    def fields(ln, label):
        f = ln.split("\t")
        assert len(f) == 11 and f[-1] == "" and int(f[0]) == label, ln
        return [int(x) for x in f[1:6]], f[6:10]

    for k, ln in enumerate(body[:2 * w]):
        c5[k], f5[k] = fields(ln, k - w)
    rev = body[2 * w + 3:]
    for k in range(w):                       # inside rows w-1 .. 0
        c3[2 * w - 1 - k], f3[2 * w - 1 - k] = fields(rev[k], w - 1 - k)
    for k in range(w):                       # outside rows labelled 1 .. w = offsets -1 .. -w
        c3[w - 1 - k], f3[w - 1 - k] = fields(rev[w + k], k + 1)
    return w, c5, c3, f5, f3

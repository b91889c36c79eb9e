"""The quality rescale (csrc/rescale_kernels.h, host/rescale.c, hostcheck -k): the definition restated in Python -- the rates-file parser, the P(damage) table, and
rescale_stream on BAM bytes.  The judge of every test of the option; nothing in it comes from the engine or the host library.

A candidate is defined through the tally: rescale_stream runs the substitution tally of one record the way
base_quality_lib.direct_pss_counts does -- the window s - 2 .. s + L + 1 in read orientation, read base i from the 5' end against
window position 2 + i for the forward table, read base L - 1 - i against L + 1 - i for the reverse table -- and whenever that tally
adds to cell (T, C) of forward row i, or to cell (A, G) (ds) / (T, C) (ss) of reverse row i, the stored position the read base came
from is a candidate of row i.  Which end of the stored SEQ, which table a mate feeds, |TLEN| and -Q all follow from that."""
import math
import struct

import numpy as np

import pssbam_testlib as tl

QUALS = 94
MAX_ROWS = 64
COLS = ["AC", "AG", "AT", "CA", "CG", "CT", "GA", "GC", "GT", "TA", "TC", "TG"]
FL_REJECT = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CELL_TC, CELL_AG = 4 * 3 + 1, 4 * 0 + 2


class Refused(ValueError):
    pass


# ---- the rates file ---------------------------------------------------------------------------------------------------------------

def parse_rates(text: str, name: str = "rates"):
    """-> (forward rows, reverse rows), each a list of 12-float lists, row 0 first.  '#' and blank lines apart a line is a position
    and twelve rates in [0, 1]; a '#' line behind rows closes their table; forward positions ascend from 0, reverse ones descend to 0."""
    tabs, pos_of, section = [[], []], [[], []], 0
    for no, line in enumerate(text.splitlines(), 1):
        f = line.split()
        if not f:
            continue
        if f[0].startswith("#"):
            if section < 2 and tabs[section]:
                section += 1
            continue
        try:
            assert len(f) == 13 and f[0].isdigit()
            pos, vals = int(f[0]), [float(v) for v in f[1:]]
            assert all(0.0 <= v <= 1.0 for v in vals)
        except (AssertionError, ValueError):
            raise Refused(f"{name} line {no}: not a position and twelve rates in [0, 1]")
        if section == 0 and pos != len(tabs[0]):
            raise Refused(f"{name} line {no}: the forward rows are not 0, 1, 2, ...")
        if section == 1 and pos_of[1] and pos != pos_of[1][0] - len(pos_of[1]):
            raise Refused(f"{name} line {no}: the reverse rows do not descend to 0")
        if section == 2:
            raise Refused(f"{name} line {no}: a row behind the two tables")
        tabs[section].append(vals)
        pos_of[section].append(pos)
    if pos_of[1] and pos_of[1][-1] != 0:
        raise Refused(f"{name}: the reverse rows do not descend to 0")
    if not tabs[0] and not tabs[1]:
        raise Refused(f"{name} holds no rows")
    if len(tabs[0]) != len(tabs[1]):
        raise Refused(f"{name}: {len(tabs[0])} forward and {len(tabs[1])} reverse rows")
    return tabs[0], tabs[1][::-1]


def unrounded(q: int, d: float) -> float:
    return -10.0 * math.log10(1.0 - (1.0 - 10.0 ** (-q / 10.0)) * (1.0 - d))


def build(text: str, mode: str, baseline=None, name: str = "rates") -> dict:
    """{"file_rows" R, "rows" min(R, 64), "baseline" [b5, b3], "rate" [2][rows], "damage" [2][rows], "table" uint8 [2][rows][94],
    "near_half": the entries whose unrounded value lies within 1e-9 of a half}"""
    assert mode in ("ds", "ss")
    if baseline is not None and not 0.0 <= baseline < 1.0:
        raise Refused(f"the baseline is a rate in [0, 1), not {baseline}")
    fwd, rev = parse_rates(text, name)
    R = len(fwd)
    rows = min(R, MAX_ROWS)
    col = [[r[COLS.index("TC")] for r in fwd], [r[COLS.index("AG" if mode == "ds" else "TC")] for r in rev]]
    out = {"file_rows": R, "rows": rows, "baseline": [], "rate": np.zeros((2, rows)), "damage": np.zeros((2, rows)),
           "table": np.zeros((2, rows, QUALS), dtype=np.uint8), "near_half": 0}
    for end in range(2):
        b = baseline
        if b is None:
            total = 0.0
            for i in range(R // 2, R):
                total += col[end][i]
            b = total / (R - R // 2)
        out["baseline"].append(b)
        for i in range(rows):
            rate = col[end][i]
            d = 1.0 - b / rate if rate > b and rate > 0.0 else 0.0
            out["rate"][end, i], out["damage"][end, i] = rate, d
            for q in range(QUALS):
                if d == 0.0:
                    out["table"][end, i, q] = q
                    continue
                x = unrounded(q, d)
                if abs(x - math.floor(x) - 0.5) < 1e-9:
                    out["near_half"] += 1
                out["table"][end, i, q] = min(q, max(0, math.floor(x + 0.5)))
    return out


def rates_text(fwd_tc, rev_ag, rev_tc=None, fill: float = 0.0) -> str:
    """a rates file as pss_write_rates prints it, with the given TC column of the forward and AG / TC columns of the reverse table"""
    rev_tc = rev_ag if rev_tc is None else rev_tc
    R = len(fwd_tc)
    assert len(rev_ag) == R == len(rev_tc)

    def row(pos, ag, tc):
        v = [fill] * 12
        v[COLS.index("AG")], v[COLS.index("TC")] = ag, tc
        return f"{pos}\t" + "".join(f"{x:.5e}\t" for x in v) + "\n"

    head = "### pss-bam.c v1.2.1\n### FASTA: g.fa\n### BAM: a.bam\n### OUT: x.pss.rates.txt\n### POS " + " ".join(COLS) + "\n"
    return (head + "### Forward read substitution rates\n" + "".join(row(i, fill, fwd_tc[i]) for i in range(R)) +
            "\n\n### Reverse read substitution rates\n" + "".join(row(i, rev_ag[i], rev_tc[i]) for i in reversed(range(R))))


def identity_table(rows: int) -> np.ndarray:
    return np.tile(np.arange(QUALS, dtype=np.uint8), (2, rows, 1))


# ---- the records ------------------------------------------------------------------------------------------------------------------

def split_records(raw) -> list:
    b = raw.tobytes() if isinstance(raw, np.ndarray) else bytes(raw)
    out, o = [], 0
    while o < len(b):
        n = 4 + struct.unpack_from("<I", b, o)[0]
        assert o + n <= len(b), "the stream ends inside a record"
        out.append(b[o:o + n])
        o += n
    return out


def rescale_record(rec: bytes, contigs: dict, ref_names: list, mode: str, table, D: int, o: tl.PssOpts, min_bq: int = 0):
    """-> (the record with its QUAL rescaled, [(end, row, lowered?)] of its candidates, tallied?).  contigs: name -> sequence text;
    D = min(rows of the table, o.region_len)."""
    block_size, ref_id, pos0, l_name, mapq, _bin, n_cig, flag, l_seq, _nref, _npos, tlen = struct.unpack_from("<IiiBBHHHIiii", rec, 0)
    seq_at = 36 + l_name + 4 * n_cig
    qual_at = seq_at + (l_seq + 1) // 2
    if len(rec) != 4 + block_size or qual_at + l_seq > len(rec):
        return rec, [], False
    seq = "".join(tl.SEQ_CODES[(rec[seq_at + i // 2] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l_seq))
    qual = rec[qual_at:qual_at + l_seq]
    has_qual = l_seq > 0 and qual[0] != 0xFF
    l_text = l_seq if l_seq else 1
    if not has_qual and l_text != 1:
        return rec, [], False                          # SEQ and QUAL differ in length as text: the line is skipped
    name = ref_names[ref_id] if 0 <= ref_id < len(ref_names) else None
    ref = contigs.get(name)
    if ref is None:
        return rec, [], False
    ref = ref.upper()
    paired = bool(flag & 1)
    L = abs(tlen) if paired else l_text
    s = pos0
    cigar = [(v >> 4, v & 15) for v in struct.unpack_from(f"<{n_cig}I", rec, 36 + l_name)]
    if s - 2 < 0 or s + L + 2 > len(ref) or cigar != [(L, 0)] or (flag & FL_REJECT):
        return rec, [], False
    if mapq < o.min_mq or not (o.min_read_len <= L <= o.max_read_len and L >= o.region_len) or (o.merged_only and paired):
        return rec, [], False
    is_rev = bool(flag & 0x10)

    def comp(c):
        return _COMP.get(c, c)

    def g(j):                                           # the window s-2 .. s+L+1 in read orientation
        return comp(ref[s - 2 + (L + 3 - j)]) if is_rev else ref[s - 2 + j]

    def stored(i):                                      # where read base i (read orientation) is stored
        return L - 1 - i if is_rev else i

    def rd(i):                                          # read base i in read orientation, None when masked / absent
        k = stored(i)
        if not 0 <= k < len(seq):
            return None
        if qual[k] < min_bq:
            return None
        c = seq[k].upper()
        return comp(c) if is_rev else c

    up_ok, dn_ok = g(1) in o.up_ctx, g(L + 2) in o.down_ctx
    if not paired:
        in_fwd = in_rev = up_ok and dn_ok
    elif (flag & 0x2) and not (flag & 0x8):
        in_fwd = bool(flag & 0x40) and up_ok
        in_rev = not in_fwd and bool(flag & 0x80) and dn_ok
    else:
        in_fwd = in_rev = False
    if not (in_fwd or in_rev):
        return rec, [], False
    want3 = CELL_AG if mode == "ds" else CELL_TC
    cands = []                                          # (end, row, stored index)
    for i in range(D):
        if in_fwd:
            a, b = rd(i), g(2 + i)
            if a in _CODE and b in _CODE and 4 * _CODE[a] + _CODE[b] == CELL_TC:
                cands.append((0, i, stored(i)))
        if in_rev:
            a, b = rd(L - 1 - i), g(L + 1 - i)
            if a in _CODE and b in _CODE and 4 * _CODE[a] + _CODE[b] == want3:
                cands.append((1, i, stored(L - 1 - i)))
    out, met = bytearray(rec), []
    for end, i, k in cands:
        q = qual[k]
        lowered = False
        if has_qual and q < QUALS:
            new = int(table[end][i][q])
            lowered = new < q
            out[qual_at + k] = min(out[qual_at + k], new)
        met.append((end, i, lowered))
    return bytes(out), met, True


def rescale_stream(raw, contigs, ref_names, mode: str, table, o: tl.PssOpts = None, min_bq: int = 0, only_tallied: bool = False):
    """raw: BAM records back to back (the whole input, or the kept records of a run: a record the tally leaves out is passed through);
    only_tallied: those are left out instead, which makes the stream the one a sink receives)
    -> (the rescaled stream, counts uint64 [2][rows][2] = candidates and lowered per end and row, the number of tallied records)"""
    o = o or tl.PssOpts()
    contigs = dict(contigs)
    rows = len(table[0])
    D = min(rows, o.region_len)
    counts = np.zeros((2, rows, 2), dtype=np.uint64)
    out, n = [], 0
    for rec in split_records(raw):
        new, met, tallied = rescale_record(rec, contigs, ref_names, mode, table, D, o, min_bq)
        n += tallied
        for end, i, lowered in met:
            counts[end, i, 0] += 1
            counts[end, i, 1] += lowered
        if tallied or not only_tallied:
            out.append(new)
    return b"".join(out), counts, n


# ---- the golden fixtures (tests/golden/make_rescale_golden.py writes them) --------------------------------------------------------

GOLDEN_MODE, GOLDEN_MIN_MQ = "ds", 20
_OFF_DIAG = [1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14]      # the cells of COLS; cell & 3 = the reference base


def pss_rates_text(fasta: str, bam: str, out_name: str, fwd, rev) -> str:
    """<prefix>.pss.rates.txt for the two count tables, as host/report.c writes it: a rate is the cell over its reference base's
    column sum, and a row in which a reference base was never seen is all zero"""
    def rates(tab):
        out = []
        for row in np.asarray(tab)[2:]:
            col = [int(row[r]) + int(row[4 + r]) + int(row[8 + r]) + int(row[12 + r]) for r in range(4)]
            out.append([0.0 if 0 in col else int(row[c]) / col[c & 3] for c in _OFF_DIAG])
        return out

    def line(pos, vals):
        return f"{pos}\t" + "".join(f"{v:.5e}\t" for v in vals) + "\n"

    f, r = rates(fwd), rates(rev)
    head = (f"### pss-bam.c v1.2.1\n### FASTA: {fasta}\n### BAM: {bam}\n### OUT: {out_name}\n### Format of table:\n"
            "### Substitution rates for all possible nucleotide substitutions at\n### each position in the aligned reads.\n"
            "### First base is what was seen in the read.\n### Second base is what was in the genome at that position.\n"
            "### POS " + " ".join(COLS) + "\n")
    return (head + "### Forward read substitution rates\n" + "".join(line(i, v) for i, v in enumerate(f)) +
            "\n\n### Reverse read substitution rates\n" + "".join(line(i, r[i]) for i in reversed(range(len(r)))))


def golden() -> dict:
    """setD under -q 20 -r 15: the rates file of that run (from base_quality_lib.direct_pss_counts, an independent count of the
    tables) and the kept records rescaled with it in mode ds"""
    from pathlib import Path

    import base_quality_lib as bq
    import mismatch_lib as ml

    gold = Path(__file__).resolve().parent / "golden"
    fa_txt = (gold / "setD.fa").read_text()
    contigs = [(blk.split("\n", 1)[0].split()[0], "".join(blk.split("\n")[1:])) for blk in fa_txt.split(">")[1:]]
    refs, raw = tl.read_bam(gold / "setD.bam")
    _, recs = ml.read_sam(gold / "setD.sam")
    o = tl.PssOpts(min_mq=GOLDEN_MIN_MQ)
    fwd, rev = bq.direct_pss_counts(contigs, recs, o, 0)
    rates = pss_rates_text("setD.fa", "setD.bam", "first.pss.rates.txt", fwd, rev)
    built = build(rates, GOLDEN_MODE, name="rescale_setD.rates.txt")
    kept, counts, n = rescale_stream(raw, contigs, [name for name, _ in refs], GOLDEN_MODE, built["table"], o, only_tallied=True)
    plain = rescale_stream(raw, contigs, [name for name, _ in refs], GOLDEN_MODE, identity_table(built["rows"]), o, only_tallied=True)[0]
    return {"rates": rates, "kept": kept, "plain": plain, "built": built, "counts": counts, "n": n, "fwd": fwd, "rev": rev,
            "contigs": contigs, "refs": refs, "raw": raw}

"""The yardstick of pss-bam -I, shared by test_gapped_host.py and test_gpu_gapped.py.

`pss-bam -I` on a file == the tool without -I on the same file after every record that ANCHORS has been replaced by
its anchored record, `<span>M` with the matched run at either end of the alignment kept and N / ! in between
(anchor_rec / anchor_recs / anchor_sam_text build that second file).  direct_counts is an independent count: it
expands the CIGAR of the ORIGINAL record into alignment columns and reads the two ends off them, and never builds an
anchored record; the transformation is checked against it once, on the CPU oracle.  fuzz_case rewrites a share of
tl.fuzz_dataset's CIGARs into clipped / gapped ones, and into the shapes that must not anchor."""
from __future__ import annotations

import re
from dataclasses import replace

import numpy as np

import pssbam_testlib as tl

MATCH_OPS = "M=X"
SPAN_MAX = (1 << 31) - 1


def anchor_info(r: tl.Rec):
    """None when the record does not anchor, else dict(span, q0, q1, a, b): the reference length of the core, the read
    offsets between the soft clips, the summed match-type runs at the core's start and end"""
    ops = r.cigar
    if not ops or any(n < 1 for n, _ in ops):
        return None
    i, j = 0, len(ops)
    clip_l = clip_r = 0
    if ops[i][1] == "H":
        i += 1
    if i < j and ops[i][1] == "S":
        clip_l = ops[i][0]
        i += 1
    if j > i and ops[j - 1][1] == "H":
        j -= 1
    if j > i and ops[j - 1][1] == "S":
        clip_r = ops[j - 1][0]
        j -= 1
    core = ops[i:j]
    if not core or any(op not in "MID=X" for _, op in core) or core[0][1] not in MATCH_OPS or core[-1][1] not in MATCH_OPS:
        return None
    if r.seq == "*" or r.qual == "*" or len(r.qual) != len(r.seq):
        return None
    if clip_l + sum(n for n, op in core if op in "MI=X") + clip_r != len(r.seq):
        return None
    span = sum(n for n, op in core if op in "MD=X")
    if span > SPAN_MAX:
        return None
    a = b = 0
    for n, op in core:
        if op not in MATCH_OPS:
            break
        a += n
    for n, op in reversed(core):
        if op not in MATCH_OPS:
            break
        b += n
    return dict(span=span, q0=clip_l, q1=len(r.seq) - clip_r, a=a, b=b)


def anchor_rec(r: tl.Rec) -> tl.Rec:
    """the anchored record of a record that anchors, the record itself otherwise"""
    an = anchor_info(r)
    if an is None:
        return r
    span, q0, q1, a, b = an["span"], an["q0"], an["q1"], an["a"], an["b"]
    if a == span:           # the whole core is match-type
        seq, qual = r.seq[q0:q1], r.qual[q0:q1]
    else:
        seq = r.seq[q0:q0 + a] + "N" * (span - a - b) + r.seq[q1 - b:q1]
        qual = r.qual[q0:q0 + a] + "!" * (span - a - b) + r.qual[q1 - b:q1]
    return replace(r, cigar=[(span, "M")], seq=seq, qual=qual)


def anchor_recs(recs: list) -> list:
    return [anchor_rec(r) for r in recs]


_CIG = re.compile(r"(\d+)([MIDNSHP=X])")


def anchor_sam_text(text: str) -> str:
    """the same on SAM text (header lines pass through, optional fields are kept)"""
    out = []
    for ln in text.splitlines(keepends=True):
        if ln.startswith("@"):
            out.append(ln)
            continue
        f = ln.rstrip("\n").split("\t")
        cigar = [] if f[5] == "*" else [(int(n), op) for n, op in _CIG.findall(f[5])]
        r = anchor_rec(tl.Rec(f[0], int(f[1]), f[2], int(f[3]), int(f[4]), cigar, seq=f[9], qual=f[10]))
        f[5], f[9], f[10] = r.cigar_str(), r.seq, r.qual
        out.append("\t".join(f) + "\n")
    return "".join(out)


# ---- the independent count ---------------------------------------------------------------------------------------

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
FL_REJECT = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
_SHAPE = re.compile(r"^(?:\d+H)?(?:(\d+)S)?((?:\d+[MID=X])+)(?:(\d+)S)?(?:\d+H)?$")


def columns(r: tl.Rec):
    """(alignment columns of the core as one letter each -- m: a read base over a reference base, i: a read base over
    nothing, d: a reference base under nothing --, leading soft clip, trailing soft clip), or None when the CIGAR text is
    not [H][S] core [S][H] over M I D = X with positive lengths, the core does not start and end with an m column, or
    the read's bases do not fill the columns"""
    text = r.cigar_str()
    m = _SHAPE.match(text)
    if not m or any(int(n) == 0 for n, _ in _CIG.findall(text)):
        return None
    cols = "".join({"M": "m", "=": "m", "X": "m", "I": "i", "D": "d"}[op] * int(n) for n, op in _CIG.findall(m.group(2)))
    lead, trail = int(m.group(1) or 0), int(m.group(3) or 0)
    if cols[0] != "m" or cols[-1] != "m":
        return None
    if r.seq == "*" or r.qual == "*" or len(r.seq) != len(r.qual):
        return None
    if lead + len(cols) - cols.count("d") + trail != len(r.seq) or len(cols) - cols.count("i") > SPAN_MAX:
        return None
    return cols, lead, trail


def direct_counts(contigs, recs, o: tl.PssOpts, q: int = 0):
    """pss-bam -I's tables (fwd, rev) counted straight from the original records: a reference position of the alignment
    is counted, by whichever end's window reaches it, when its column is m and no i / d column lies between it and the
    alignment's first column, or none between it and the last; -Q q leaves out the positions whose read base has a
    quality below q.  Restates process_aln's filters with the reference length of the
    alignment in the CIGAR's place; a record whose CIGAR is not of the clipped / gapped shape falls under the plain rule."""
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
        shape = columns(r)
        if shape is not None:
            cols, lead, trail = shape
            span = len(cols) - cols.count("i")
            run_l = len(cols) - len(cols.lstrip("m"))
            run_r = len(cols) - len(cols.rstrip("m"))
            # read offset of the read base over each reference position, None where the column is not anchored
            over, k = [], lead
            for c, ch in enumerate(cols):
                if ch != "i":
                    over.append(k if ch == "m" and (c < run_l or c >= len(cols) - run_r) else None)
                k += ch != "d"
            L = abs(r.tlen) if paired else span
            if L != span:
                continue
        else:
            L = abs(r.tlen) if paired else len(r.seq)
            if r.cigar_str() != f"{L}M":
                continue
            over = list(range(L))
        s = r.pos - 1
        if s - 2 < 0 or s + L - 1 + 2 > len(ref) - 1:
            continue
        if r.mapq < o.min_mq or not (o.min_read_len <= L <= o.max_read_len and L >= n):
            continue
        if (r.flag & FL_REJECT) or (o.merged_only and paired):
            continue
        is_rev = bool(r.flag & 0x10)

        def base(k):                                    # read base at read offset k, None when masked / absent / unanchored
            if k is None or not 0 <= k < len(r.seq) or (r.qual != "*" and ord(r.qual[k]) - 33 < q):
                return None
            return r.seq[k].upper()

        # the two ends in reference orientation: (context2, context1, [(read base, reference base)] from the end inwards)
        left = (ref[s - 2], ref[s - 1], [(base(over[i]), ref[s + i]) for i in range(n)])
        right = (ref[s + L + 1], ref[s + L], [(base(over[L - 1 - i]), ref[s + L - 1 - i]) for i in range(n)])
        up1, dn1 = (right[1], left[1]) if is_rev else (left[1], right[1])
        if is_rev:
            up1, dn1 = _COMP.get(up1, up1), _COMP.get(dn1, dn1)
        up_ok, dn_ok = up1 in o.up_ctx, dn1 in o.down_ctx

        def tally(tab, end):
            c2, c1, pairs = end
            for row, c in ((0, c2), (1, c1)):
                if c in _CODE:
                    k = 5 * _CODE[c]
                    tab[row, 15 - k if is_rev else k] += 1
            for i, (a, b) in enumerate(pairs):
                if a in _CODE and b in _CODE:
                    k = 4 * _CODE[a] + _CODE[b]
                    tab[i + 2, 15 - k if is_rev else k] += 1

        end5, end3 = (right, left) if is_rev else (left, right)    # the forward table takes the 5' end
        if not paired:
            if up_ok and dn_ok:
                tally(fwd, end5)
                tally(rev, end3)
        elif (r.flag & 0x2) and not (r.flag & 0x8):
            if (r.flag & 0x40) and up_ok:
                tally(fwd, end5)
            elif (r.flag & 0x80) and dn_ok:
                tally(rev, end3)
    return fwd, rev


# ---- the fuzzer ----------------------------------------------------------------------------------------------------

REASONS = ("interior_S", "N", "P", "zero_len", "core_starts_gap", "core_ends_gap", "query_off_by_one", "qual_absent")


def _split(rng, total: int, parts: int) -> list:
    """`parts` positive integers that sum to `total` (total >= parts)"""
    cuts = np.sort(rng.choice(np.arange(1, total), size=parts - 1, replace=False)) if parts > 1 else np.array([], dtype=int)
    edges = [0] + [int(c) for c in cuts] + [total]
    return [edges[k + 1] - edges[k] for k in range(parts)]


def _gapped_cigar(rng, qlen: int) -> list:
    """an anchoring CIGAR over qlen read bases: clips at either or both extremes, none or 2..12 interior I / D ops, = / X
    runs next to M, terminal runs of 1..70 bases"""
    clip_l = int(rng.integers(1, max(2, min(qlen // 3, 40)))) if rng.random() < 0.45 and qlen >= 6 else 0
    clip_r = int(rng.integers(1, max(2, min(qlen // 3, 40)))) if rng.random() < 0.45 and qlen - clip_l >= 6 else 0
    body = qlen - clip_l - clip_r
    k = int(rng.integers(2, 13)) if rng.random() < 0.6 else 0
    while k and body < 2 * k + 1:
        k -= 1
    core = []
    if k == 0:
        core = [(body, "M=X"[int(rng.integers(0, 3))])] if rng.random() < 0.5 or body < 2 else \
            [(n, op) for n, op in zip(_split(rng, body, 2), ("M", "=") if rng.random() < 0.5 else ("X", "M"))]
    else:
        kinds = ["ID"[int(x)] for x in rng.integers(0, 2, size=k)]
        ins = [int(rng.integers(1, 4)) if kd == "I" else 0 for kd in kinds]
        while sum(ins) + k + 1 > body:                  # too many inserted bases for the read: turn insertions into deletions
            j = ins.index(max(ins))
            ins[j], kinds[j] = 0, "D"
        matched = body - sum(ins)
        a = int(rng.integers(1, min(70, matched - k) + 1))
        b = int(rng.integers(1, min(70, matched - a - (k - 1)) + 1)) if k >= 1 else 0
        mids = _split(rng, matched - a - b, k - 1) if k > 1 else []
        if k == 1:
            b = matched - a
        runs = [a] + mids + [b]
        for t in range(k):
            core.append((runs[t], "M=X"[int(rng.integers(0, 3))] if rng.random() < 0.3 else "M"))
            core.append((ins[t], "I") if kinds[t] == "I" else (int(rng.integers(1, 6)), "D"))
        core.append((runs[k], "M"))
        if rng.random() < 0.3 and core[0][0] >= 2:      # the leading run as two match-type ops
            n0 = core[0][0]
            c = int(rng.integers(1, n0))
            core[0:1] = [(c, "="), (n0 - c, "M")]
    ops = [(int(rng.integers(1, 30)), "H")] if rng.random() < 0.2 else []
    ops += [(clip_l, "S")] if clip_l else []
    ops += core
    ops += [(clip_r, "S")] if clip_r else []
    ops += [(int(rng.integers(1, 30)), "H")] if rng.random() < 0.2 else []
    return ops


def _broken(rng, r: tl.Rec, why: str) -> tl.Rec:
    """the record with a CIGAR (or QUAL) that must not anchor for the one given reason"""
    q = len(r.seq)                                      # (>= 8)
    a = int(rng.integers(1, q - 2))
    if why == "interior_S":
        c = int(rng.integers(1, q - a))                 # a + c <= q - 1: a match run is left behind the clip
        return replace(r, cigar=[(a, "M"), (c, "S"), (q - a - c, "M")])
    if why == "N":
        return replace(r, cigar=[(a, "M"), (int(rng.integers(1, 50)), "N"), (q - a, "M")])
    if why == "P":
        return replace(r, cigar=[(a, "M"), (2, "P"), (q - a, "M")])
    if why == "zero_len":
        return replace(r, cigar=[(a, "M"), (0, "ID"[int(rng.integers(0, 2))]), (q - a, "M")] if rng.random() < 0.7 else [(0, "S"), (q, "M")])
    if why == "core_starts_gap":
        return replace(r, cigar=[(2, "S"), (a, "I"), (q - a - 2, "M")] if rng.random() < 0.5 else [(3, "D"), (q, "M")])
    if why == "core_ends_gap":
        return replace(r, cigar=[(q - a, "M"), (a, "I")] if rng.random() < 0.5 else [(q, "M"), (2, "D"), (4, "H")])
    if why == "query_off_by_one":
        return replace(r, cigar=[(a, "M"), (2, "D"), (q - a + (1 if rng.random() < 0.5 else -1), "M")])
    assert why == "qual_absent"
    return replace(r, cigar=[(a, "M"), (1, "D"), (q - a, "M")], qual="*")


def fuzz_case(seed: int, n: int = 3000, with_rg: bool = False):
    """(contigs, refs, recs, why): tl.fuzz_dataset(seed, n) with 55 % of the records that carry bases given an anchoring
    clipped / gapped CIGAR over the same SEQ / QUAL and 14 % one that must not anchor; why[i] is None or the reason
    record i was broken for.  A third of the paired ones among the rewritten get |TLEN| == span."""
    contigs, refs, recs = tl.fuzz_dataset(seed, n, with_rg=with_rg)
    rng = np.random.default_rng(seed + 77)
    lens = dict(refs)
    out, why = [], []
    for r in recs:
        u = rng.random()
        q = len(r.seq)
        if r.seq == "*" or q < 8 or u >= 0.69:
            out.append(r)
            why.append(None)
            continue
        if r.qual == "*":
            r = replace(r, qual="".join(chr(33 + int(x)) for x in rng.integers(2, 42, size=q)))
        if u < 0.55:
            nr = replace(r, cigar=_gapped_cigar(rng, q))
            why.append(None)
        else:
            reason = REASONS[int(rng.integers(0, 2))] if u < 0.65 else REASONS[int(rng.integers(2, len(REASONS)))]
            nr = _broken(rng, r, reason)
            why.append(reason)
        span = nr.ref_span()
        # keep most rewritten alignments inside their contig (deletions lengthen them)
        if nr.rname in lens and nr.pos - 1 + span + 2 > lens[nr.rname] and rng.random() < 0.8:
            nr = replace(nr, pos=max(1, lens[nr.rname] - span - 2 - int(rng.integers(0, 4)) + 1))
        if nr.flag & 1:
            t = rng.random()
            if t < 0.6:
                nr = replace(nr, tlen=span if t < 0.3 else -span)
        out.append(nr)
    return contigs, refs, out, why

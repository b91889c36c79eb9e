"""The definition of duplicate flagging (pssbam_engine_set_duplicates, pss-bam -d, fragkon -d) restated in Python: which records
are eligible, their keys, which of them are duplicates, the totals and the group-size histogram.  It works on tl.Rec lists and on
raw BAM records alike, through one neutral view of a record (Core).

  eligible   unpaired; not dropped by the read-group filter; not a parse skip; contig in the genome; none of 0x4 0x100 0x200
             0x400 0x800; POS given; CIGAR exactly <L>M with L the SEQ length ('*' counts 1); the tool's mapping quality, length
             window and contig margin (pss: two bases either side and L >= -r; fragkon: k/2 either side); the regions when set
  key        (refID, POS, L, FLAG & 0x10, g), g = 1 + the index of the record's first RG:Z value among the groups, 0 without
  duplicate  an eligible record with an earlier eligible record of the same key, in input order
"""
import struct
from dataclasses import dataclass, replace
from pathlib import Path

import numpy as np

import pssbam_testlib as tl

GOLD = Path(__file__).resolve().parent / "golden"
FLAG_DUP = 0x400
FL_REJECT = 0x4 | 0x100 | 0x200 | 0x400 | 0x800
HIST_MAX = 255


@dataclass
class Core:
    ref: int            # refID, -1 for '*' or a name the header lacks
    pos0: int           # 0-based POS
    mapq: int
    flag: int
    cigar: list         # [(len, op)]
    l_text: int         # strlen(SEQ): the SEQ length, 1 for '*'
    parse_skip: bool    # SEQ and QUAL of different lengths (QUAL absent beside a SEQ that is not one character long)
    rg: str | None      # the first RG:Z value


@dataclass
class Setup:
    """what eligibility depends on beside the record: the engine's tool and filters"""
    refs: list                      # [(name, length)] of the BAM header
    contigs: dict                   # name -> length of the genome's contigs
    pss: tl.PssOpts | None = None   # a PSSBAM_TALLY_PSS engine ...
    fk: tl.FkOpts | None = None     # ... or a PSSBAM_TALLY_KMER one
    read_group: str | None = None   # -R
    groups: list | None = None      # -G: the @RG IDs
    regions: dict | None = None     # -T: contig name -> [(start, end)] 0-based half open


def core_of_rec(r: tl.Rec, ref_index: dict) -> Core:
    rg = next((str(v) for t, ty, v in r.tags if t == "RG" and ty == "Z"), None)
    l_text = 1 if r.seq == "*" else len(r.seq)
    return Core(ref_index.get(r.rname, -1) if r.rname != "*" else -1, r.pos - 1, r.mapq & 0xFF, r.flag & 0xFFFF, list(r.cigar), l_text,
                r.seq != "*" and r.qual == "*" and l_text != 1, rg)


def _first_rg(aux: bytes) -> str | None:
    o = 0
    while o + 3 <= len(aux):
        tag, ty = aux[o:o + 2], chr(aux[o + 2])
        o += 3
        if ty in "AcC":
            o += 1
        elif ty in "sS":
            o += 2
        elif ty in "iIf":
            o += 4
        elif ty in "ZH":
            end = aux.find(b"\0", o)
            if end < 0:
                return None
            if tag == b"RG" and ty == "Z":
                return aux[o:end].decode("latin-1")
            o = end + 1
        elif ty == "B":
            if o + 5 > len(aux):
                return None
            sub, cnt = chr(aux[o]), struct.unpack_from("<I", aux, o + 1)[0]
            o += 5 + cnt * (1 if sub in "cC" else 2 if sub in "sS" else 4)
        else:
            return None
    return None


def core_of_raw(b: bytes) -> Core:
    """b: one well-formed BAM record with its block_size word"""
    ref, pos0, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", b, 4)
    o = 36 + l_name
    cigar = [(v >> 4, tl.CIGAR_OPS[v & 15]) for v in struct.unpack_from(f"<{n_cig}I", b, o)]
    q = o + 4 * n_cig + (l_seq + 1) // 2
    l_text = l_seq if l_seq else 1
    no_qual = l_seq == 0 or b[q] == 0xFF
    return Core(ref, pos0, mapq, flag, cigar, l_text, no_qual and l_text != 1, _first_rg(b[q + l_seq:]))


def split_raw(raw) -> list[bytes]:
    buf, out, o = bytes(raw), [], 0
    while o < len(buf):
        n = 4 + struct.unpack_from("<I", buf, o)[0]
        out.append(buf[o:o + n])
        o += n
    return out


def eligible(c: Core, s: Setup) -> bool:
    if c.flag & 0x1:
        return False
    if s.read_group is not None and c.rg != s.read_group:
        return False
    if c.parse_skip:
        return False
    name = s.refs[c.ref][0] if 0 <= c.ref < len(s.refs) else "*" if c.ref == -1 else None
    if name is None or name not in s.contigs:
        return False
    glen = s.contigs[name]
    L = c.l_text
    if (c.flag & FL_REJECT) or c.pos0 < 0 or c.cigar != [(L, "M")]:
        return False
    if s.pss is not None:
        o, margin = s.pss, 2
        if L < o.region_len:
            return False
    else:
        o, margin = s.fk, s.fk.klen // 2
    if not (c.pos0 >= margin and c.pos0 + L + margin <= glen):
        return False
    if c.mapq < o.min_mq or not (o.min_read_len <= L <= o.max_read_len):
        return False
    if s.regions is not None and not any(a < c.pos0 + L and c.pos0 < b for a, b in s.regions.get(name, [])):
        return False
    return True


def key_of(c: Core, s: Setup) -> tuple:
    g = 0
    if s.groups is not None and c.rg in s.groups:
        g = 1 + s.groups.index(c.rg)
    return (c.ref, c.pos0, c.l_text, c.flag & 0x10, g)


@dataclass
class Verdict:
    eligible: np.ndarray   # bool per record
    dup: np.ndarray        # bool per record: gets FLAG 0x400
    totals: dict           # {"eligible", "distinct", "flagged"}
    hist: np.ndarray       # hist_max + 2 words, as pssbam_engine_finish_duplicates fills them


def judge(cores: list[Core], s: Setup, hist_max: int = HIST_MAX) -> Verdict:
    el = np.zeros(len(cores), dtype=bool)
    dup = np.zeros(len(cores), dtype=bool)
    count: dict = {}
    for i, c in enumerate(cores):
        if not eligible(c, s):
            continue
        el[i] = True
        k = key_of(c, s)
        dup[i] = k in count
        count[k] = count.get(k, 0) + 1
    hist = np.zeros(hist_max + 2, dtype=np.uint64)
    for n in count.values():
        hist[min(n, hist_max + 1)] += 1
    return Verdict(el, dup, {"eligible": int(el.sum()), "distinct": len(count), "flagged": int(dup.sum())}, hist)


def judge_recs(recs: list, s: Setup, hist_max: int = HIST_MAX) -> Verdict:
    idx = {n: i for i, (n, _) in enumerate(s.refs)}
    return judge([core_of_rec(r, idx) for r in recs], s, hist_max)


def judge_raw(raw, s: Setup, hist_max: int = HIST_MAX) -> Verdict:
    return judge([core_of_raw(b) for b in split_raw(raw)], s, hist_max)


def flag_recs(recs: list, dup) -> list:
    return [replace(r, flag=r.flag | FLAG_DUP) if d else r for r, d in zip(recs, dup)]


def flag_raw(raw, dup) -> np.ndarray:
    out = np.array(np.frombuffer(bytes(raw), dtype=np.uint8))
    o = 0
    for d in dup:
        if d:
            out[o + 19] |= 0x04
        o += 4 + int(out[o:o + 4].view("<u4")[0])
    return out


def report_text(fasta: str, bam: str, totals: dict, hist, hist_max: int = HIST_MAX) -> str:
    """<prefix>.<tool>.duplicates.txt as host/duplicates.c writes it"""
    e, k, f = totals["eligible"], totals["distinct"], totals["flagged"]
    lines = ["# duplicates among the unpaired candidate reads: same contig, position, length, strand and read group; the first in input order is kept",
             f"# FASTA: {fasta}", f"# BAM: {bam}", f"eligible_reads\t{e}", f"distinct_keys\t{k}", f"flagged_reads\t{f}",
             "duplicate_fraction\t%.6f" % (f / e if e else 0.0), "size\tgroups"]
    lines += [f"{c}\t{int(hist[c])}" for c in range(1, hist_max + 1)] + [f">{hist_max}\t{int(hist[hist_max + 1])}"]
    return "\n".join(lines) + "\n"


def read_fasta(path) -> list:
    out = []
    for blk in Path(path).read_text().split(">")[1:]:
        head, *body = blk.split("\n")
        out.append((head.split()[0], "".join(body)))
    return out


def golden_input():
    """(Setup, raw records) behind tests/golden/duplicates_setD.txt: setD.bam's records, then every third of them again, then
    every fifth; pss-bam's default options"""
    refs, raw = tl.read_bam(GOLD / "setD.bam")
    blobs = split_raw(raw)
    raw2 = np.frombuffer(b"".join(blobs + blobs[::3] + blobs[::5]), dtype=np.uint8)
    contigs = {n: len(s) for n, s in read_fasta(GOLD / "setD.fa")}
    return Setup(refs, contigs, pss=tl.PssOpts()), raw2


def with_copies(recs: list, seed: int, max_copies: int = 5, shuffle: bool = False) -> list:
    """every record repeated 0..max_copies more times; a copy keeps coordinates, flags, CIGAR and tags but gets a name of its own
    and other qualities (where it has any), and lands anywhere behind its original -- or, shuffled, anywhere at all"""
    rng = np.random.default_rng(seed)
    out = []
    for i, r in enumerate(recs):
        out.append((float(i), r))
        for c in range(int(rng.integers(0, max_copies + 1))):
            q = r.qual if r.qual == "*" else "".join(chr(33 + int(v)) for v in rng.integers(2, 42, size=len(r.qual)))
            out.append((i + float(rng.random()) * (len(recs) - i), replace(r, qname=f"{r.qname[:240]}.c{c}", qual=q)))   # (l_read_name is a byte)
    if shuffle:
        order = rng.permutation(len(out))
        return [out[j][1] for j in order]
    return [r for _, r in sorted(out, key=lambda t: t[0])]

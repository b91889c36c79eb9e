"""The definition of the depth of coverage of the kept records (pssbam_engine_set_coverage, pss-bam -c / -b) restated in Python and
numpy.  It works on tl.Rec lists and on raw BAM records alike, through duplicates_lib's neutral view of a record plus TLEN.

  kept      a record added to the forward or the reverse main table: exactly what a record sink delivers and -O writes.  From raw
            kept records (the sink's, or those read back from kept.bam) nothing more is asked: every one of them counts.  For Rec
            lists `kept()` restates the candidate test of the substitution tally, paired reads included; it is the whole decision
            when both context sets hold every letter of the genome and no filter that looks at the bases is set.
  span      contig refID, positions POS .. POS + L - 1, L = the length of the <L>M CIGAR (for a kept record also the length in the
            tables, and the SEQ length unless a paired record's SEQ disagrees with its CIGAR and TLEN)
  depth     per contig: a difference array (+1 at POS, -1 at POS + L) and its cumulative sum
  summary   per reference of the header that the genome holds {covered, depth_sum, max_depth}; the histogram of depth 0..255 and
            above over those contigs, each once; the maximal runs of equal non-zero depth, by refID then start, half-open
"""
import struct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import duplicates_lib as dl
import pssbam_testlib as tl

GOLD = Path(__file__).resolve().parent / "golden"
HIST_MAX = 255


@dataclass
class Core(dl.Core):
    tlen: int = 0


def core_of_rec(r: tl.Rec, ref_index: dict) -> Core:
    return Core(**vars(dl.core_of_rec(r, ref_index)), tlen=r.tlen)


def core_of_raw(b: bytes) -> Core:
    return Core(**vars(dl.core_of_raw(b)), tlen=struct.unpack_from("<i", b, 32)[0])


def kept(c: Core, s: dl.Setup) -> bool:
    """the candidate test of the substitution tally (s.pss), for unpaired and paired records"""
    o = s.pss
    if s.read_group is not None and c.rg != s.read_group:
        return False
    if c.parse_skip:
        return False
    name = s.refs[c.ref][0] if 0 <= c.ref < len(s.refs) else "*" if c.ref == -1 else None
    if name is None or name not in s.contigs:
        return False
    glen = s.contigs[name]
    paired = bool(c.flag & 0x1)
    L = abs(c.tlen) if paired else c.l_text
    if (c.flag & dl.FL_REJECT) or c.pos0 < 0 or c.cigar != [(L, "M")]:
        return False
    if not (c.pos0 >= 2 and c.pos0 + L + 2 <= glen):
        return False
    if c.mapq < o.min_mq or not (o.min_read_len <= L <= o.max_read_len) or L < o.region_len:
        return False
    if paired and (o.merged_only or (c.flag & 0xA) != 0x2 or not (c.flag & 0xC0)):   # proper, mate mapped, a mate number
        return False
    if s.regions is not None and not any(a < c.pos0 + L and c.pos0 < b for a, b in s.regions.get(name, [])):
        return False
    return True


def span(c: Core) -> tuple:
    """(refID, POS, L) of a kept record"""
    assert len(c.cigar) == 1 and c.cigar[0][1] == "M", c
    return c.ref, c.pos0, c.cigar[0][0]


@dataclass
class Summary:
    per_contig: np.ndarray   # n_ref x {covered, depth_sum, max_depth}, uint64; zero for a reference the genome lacks
    hist: np.ndarray         # HIST_MAX + 2 words: positions at depth 0..HIST_MAX, then above
    runs: tuple              # (ref int32, start uint32, end uint32, depth uint32)
    depths: list             # per reference: its depth array (int64), or None when the genome lacks it

    @property
    def n_runs(self) -> int:
        return len(self.runs[0])


def depth_arrays(spans, refs: list, contigs: dict) -> list:
    """per reference of the header: the depth at every position of the genome's contig of that name (difference, cumulative
    sum), None when the genome has none; a name the header lists twice counts under its first refID"""
    first = {}
    for i, (n, _) in enumerate(refs):
        first.setdefault(n, i)
    diff = [np.zeros(contigs[n] + 1, dtype=np.int64) if n in contigs and first[n] == i else None for i, (n, _) in enumerate(refs)]
    for ref, pos0, L in spans:
        d = diff[first[refs[ref][0]]]
        assert d is not None and 0 <= pos0 and pos0 + L <= len(d) - 1, (ref, pos0, L)
        d[pos0] += 1
        d[pos0 + L] -= 1
    return [None if d is None else np.cumsum(d)[:-1] for d in diff]


def summarise(depths: list, hist_max: int = HIST_MAX) -> Summary:
    per = np.zeros((len(depths), 3), dtype=np.uint64)
    hist = np.zeros(hist_max + 2, dtype=np.uint64)
    rr, rs, re_, rd = [], [], [], []
    for i, d in enumerate(depths):
        if d is None:
            continue
        per[i] = (int((d > 0).sum()), int(d.sum()), int(d.max()) if d.size else 0)
        hist += np.bincount(np.minimum(d, hist_max + 1), minlength=hist_max + 2).astype(np.uint64)
        if not d.size:
            continue
        edge = np.flatnonzero(np.diff(d)) + 1                    # where the depth changes
        starts = np.concatenate(([0], edge))
        ends = np.concatenate((edge, [d.size]))
        keep = d[starts] > 0
        rr.append(np.full(int(keep.sum()), i, dtype=np.int32))
        rs.append(starts[keep])
        re_.append(ends[keep])
        rd.append(d[starts][keep])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)  # noqa: E731
    return Summary(per, hist, (cat(rr, np.int32), cat(rs, np.uint32), cat(re_, np.uint32), cat(rd, np.uint32)), depths)


def from_spans(spans, refs: list, contigs: dict, hist_max: int = HIST_MAX) -> Summary:
    return summarise(depth_arrays(spans, refs, contigs), hist_max)


def from_raw(raw_kept, refs: list, contigs: dict, hist_max: int = HIST_MAX) -> Summary:
    """raw_kept: the kept records, as the record sink delivers them or as they stand in kept.bam -- no further filter"""
    return from_spans([span(core_of_raw(b)) for b in dl.split_raw(raw_kept)], refs, contigs, hist_max)


def from_recs(recs: list, s: dl.Setup, hist_max: int = HIST_MAX) -> Summary:
    idx = {n: i for i, (n, _) in enumerate(s.refs)}
    cores = [core_of_rec(r, idx) for r in recs]
    return from_spans([span(c) for c in cores if kept(c, s)], s.refs, s.contigs, hist_max)


def same(a: Summary, per_contig, hist, runs) -> bool:
    return (np.array_equal(a.per_contig, per_contig) and np.array_equal(a.hist, hist) and len(runs) == 4 and
            all(np.array_equal(x, np.asarray(y)) for x, y in zip(a.runs, runs)))


def coverage_text(fasta: str, bam: str, refs: list, contigs: dict, s: Summary, hist_max: int = HIST_MAX) -> str:
    """<prefix>.pss.coverage.txt as host/coverage.c writes it"""
    lines = ["# depth of coverage of the tallied reads: every read added to a table covers POS .. POS + length - 1 of its contig",
             f"# FASTA: {fasta}", f"# BAM: {bam}", "contig\tlength\tcovered_bases\tbreadth\tdepth_sum\tmean_depth\tmax_depth"]
    t = [0, 0, 0, 0]
    for i, (n, _) in enumerate(refs):
        if n not in contigs:
            continue
        ln, (cov, dsum, dmax) = contigs[n], (int(v) for v in s.per_contig[i])
        lines.append("%s\t%d\t%d\t%.6f\t%d\t%.6f\t%d" % (n, ln, cov, cov / ln if ln else 0.0, dsum, dsum / ln if ln else 0.0, dmax))
        t = [t[0] + ln, t[1] + cov, t[2] + dsum, max(t[3], dmax)]
    lines.append("total\t%d\t%d\t%.6f\t%d\t%.6f\t%d" % (t[0], t[1], t[1] / t[0] if t[0] else 0.0, t[2], t[2] / t[0] if t[0] else 0.0, t[3]))
    lines.append("depth\tpositions")
    lines += [f"{d}\t{int(s.hist[d])}" for d in range(hist_max + 1)] + [f">{hist_max}\t{int(s.hist[hist_max + 1])}"]
    return "\n".join(lines) + "\n"


def bedgraph_text(refs: list, runs) -> str:
    return "".join(f"{refs[int(r)][0]}\t{int(a)}\t{int(b)}\t{int(d)}\n" for r, a, b, d in zip(*runs))


def kept_of_golden():
    """(refs, contigs, spans) behind tests/golden/coverage_setD.*: setD.bam's records that pss-bam's default options keep by the
    candidate test, each of them three times over at every fifth record (so that the depth passes 1)"""
    refs, raw = tl.read_bam(GOLD / "setD.bam")
    contigs = {n: len(s) for n, s in dl.read_fasta(GOLD / "setD.fa")}
    s = dl.Setup(refs, contigs, pss=tl.PssOpts())
    cores = [core_of_raw(b) for b in dl.split_raw(raw)]
    spans = [span(c) for c in cores if kept(c, s)]
    return refs, contigs, spans + spans[::5] + spans[::5]

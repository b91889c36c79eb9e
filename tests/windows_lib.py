"""The definition of pss-bam -w (pssbam_engine_finish_coverage_windows) restated in Python and numpy, on top of coverage_lib's depth
arrays.

  windows   every reference of the header that the genome holds (a name listed twice: under its first refID) is cut into
            [k W, min((k + 1) W, length)), k = 0 .. ceil(length / W) - 1, contig-relative and 0-based; by refID, then start
  acgt      the window's positions whose FASTA letter, upper-cased, is A, C, G or T;  gc: those that are C or G
  covered   its positions at depth > 0;  depth_sum: the sum of its depths
  GC bias   a window is used when end - start == W and 2 acgt >= W; its bin is (200 gc + acgt) // (2 acgt), the GC percentage
            rounded half up; per bin the used windows, their positions (windows x W) and their summed depth
"""
import numpy as np

import coverage_lib as cl

W_MIN, W_MAX, GC_BINS = 16, 1 << 30, 101
NAMES = ("ref", "start", "end", "acgt", "gc", "covered", "depth_sum")
DTYPES = (np.int32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint64)


def windows(depths: list, refs: list, seqs: dict, W: int) -> tuple:
    """depths: coverage_lib.depth_arrays' list (None for a reference without windows); seqs: contig name -> its letters.
    -> (ref, start, end, acgt, gc, covered, depth_sum)"""
    assert W_MIN <= W <= W_MAX
    parts = [[] for _ in NAMES]
    for i, d in enumerate(depths):
        if d is None or not d.size:
            continue
        letters = np.frombuffer(seqs[refs[i][0]].upper().encode(), dtype=np.uint8)
        assert letters.size == d.size
        edges = np.arange(0, d.size, W, dtype=np.int64)
        is_gc = np.isin(letters, np.frombuffer(b"CG", dtype=np.uint8))
        is_acgt = is_gc | np.isin(letters, np.frombuffer(b"AT", dtype=np.uint8))
        cols = (np.full(edges.size, i), edges, np.minimum(edges + W, d.size), np.add.reduceat(is_acgt.astype(np.int64), edges),
                np.add.reduceat(is_gc.astype(np.int64), edges), np.add.reduceat((d > 0).astype(np.int64), edges), np.add.reduceat(d.astype(np.int64), edges))
        for p, c in zip(parts, cols):
            p.append(c)
    return tuple(np.concatenate(p).astype(dt) if p else np.zeros(0, dtype=dt) for p, dt in zip(parts, DTYPES))


def from_spans(spans, refs: list, seqs: dict, W: int) -> tuple:
    return windows(cl.depth_arrays(spans, refs, {n: len(s) for n, s in seqs.items()}), refs, seqs, W)


def from_raw(raw_kept, refs: list, seqs: dict, W: int) -> tuple:
    """raw_kept: the kept records, as the record sink delivers them or as they stand in kept.bam -- no further filter"""
    return from_spans([cl.span(cl.core_of_raw(b)) for b in cl.dl.split_raw(raw_kept)], refs, seqs, W)


def same(a: tuple, b: tuple) -> bool:
    return len(a) == len(b) == 7 and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def gcbias_rows(W: int, win: tuple) -> tuple:
    """-> (windows per bin, depth_sum per bin, used windows)"""
    _, start, end, acgt, gc, _, dsum = (np.asarray(v).tolist() for v in win)   # (Python integers: no overflow)
    bw, bs = [0] * GC_BINS, [0] * GC_BINS
    used = 0
    for s, e, a, g, d in zip(start, end, acgt, gc, dsum):
        if e - s != W or 2 * a < W or a == 0 or g > a:                       # (g > a: never from the engine; no bin beyond 100)
            continue
        b = int((200 * g + a) // (2 * a))
        bw[b] += 1
        bs[b] += int(d)
        used += 1
    return bw, bs, used


def windows_text(fasta: str, bam: str, refs: list, W: int, win: tuple) -> str:
    """<prefix>.pss.windows.txt as host/windows.c writes it"""
    lines = ["# fixed windows over the depth of coverage of the tallied reads: the FASTA's A/C/G/T and C/G letters, the covered positions and the "
             "summed depth of each", f"# FASTA: {fasta}", f"# BAM: {bam}", f"# window: {W}", f"# windows: {len(win[0])}",
             "contig\tstart\tend\tacgt\tgc\tgc_fraction\tcovered\tdepth_sum\tmean_depth"]
    for r, s, e, a, g, c, d in zip(*(v.tolist() for v in win)):
        frac = "%.6f" % (g / a) if a else "NA"
        lines.append("%s\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%.6f" % (refs[r][0], s, e, a, g, frac, c, d, d / (e - s)))
    return "\n".join(lines) + "\n"


def gcbias_text(fasta: str, bam: str, W: int, win: tuple) -> str:
    """<prefix>.pss.gcbias.txt as host/windows.c writes it"""
    bw, bs, used = gcbias_rows(W, win)
    overall = sum(bs) / (used * W) if used else 0.0
    lines = ["# GC bias of the tallied reads: the windows of the full size with at least half of their letters A, C, G or T, by the GC percentage "
             "of those letters (rounded half up)", f"# FASTA: {fasta}", f"# BAM: {bam}", f"# window: {W}", f"# windows: {len(win[0])}",
             f"# used windows: {used}", "# mean depth of the used windows: %.6f" % overall,
             "gc_percent\twindows\tpositions\tdepth_sum\tmean_depth\trelative_depth"]
    for b in range(GC_BINS):
        mean = bs[b] / (bw[b] * W) if bw[b] else 0.0
        lines.append("%d\t%d\t%d\t%d\t%.6f\t%.6f" % (b, bw[b], bw[b] * W, bs[b], mean, mean / overall if overall > 0.0 else 0.0))
    return "\n".join(lines) + "\n"


GOLDEN_W = 64   # tests/golden/windows_setD.*: full and short windows, several non-empty GC bins (make_windows_golden.py checks it)


def golden():
    """(refs, seqs, spans) behind tests/golden/windows_setD.*: coverage_lib.kept_of_golden with the contigs' letters"""
    refs, _, spans = cl.kept_of_golden()
    return refs, dict(cl.dl.read_fasta(cl.GOLD / "setD.fa")), spans

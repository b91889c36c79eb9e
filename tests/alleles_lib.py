"""The definition of the strand-split allele counts at listed sites (pssbam_engine_set_sites, pss-bam -a / -t) restated in Python and
numpy, over raw BAM records: the kept records as a record sink delivers them, or as they stand in kept.bam -- no further filter.

  site      (contig name, 0-based position); resolved = on a contig that the header lists and the genome holds, below the contig's
            length; duplicates merge; a name the header lists twice counts under its first refID; order: refID, then position
  window    a kept record with start s and L = the length of its <L>M CIGAR shows, at every resolved site p of its contig with
            s + t <= p < s + L - t, the stored SEQ base at offset p - s (t = the trim); 2t >= L shows nothing
  counter   [strand][code]: strand = FLAG 0x10; code = A C G T (nibbles 1 2 4 8) or other: every other nibble, with a minimum base
            quality a base whose QUAL is below it (absent QUAL, 0xFF, never is), an offset at or beyond l_seq
  report    <prefix>.pss.alleles.txt as host/alleles.c writes it; the sites file as it reads it
"""
import struct
from dataclasses import dataclass
from pathlib import Path

import numpy as np

import coverage_lib as cl
import duplicates_lib as dl
import pssbam_testlib as tl

GOLD = Path(__file__).resolve().parent / "golden"
CODE_OF_NIBBLE = np.array([4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4], dtype=np.int64)
COLUMNS = ("fA", "fC", "fG", "fT", "fO", "rA", "rC", "rG", "rT", "rO")
MAX_TRIM = 65535


@dataclass
class Read:
    ref: int
    pos0: int
    L: int              # the length of the <L>M CIGAR
    rev: bool
    nib: np.ndarray     # l_seq SEQ nibbles
    qual: np.ndarray    # l_seq QUAL bytes


def read_of_raw(b: bytes) -> Read:
    c = cl.core_of_raw(b)
    ref, pos0, L = cl.span(c)
    l_name, n_cig, l_seq = b[12], struct.unpack_from("<H", b, 16)[0], struct.unpack_from("<I", b, 20)[0]
    o = 36 + l_name + 4 * n_cig
    packed = np.frombuffer(b, dtype=np.uint8, count=(l_seq + 1) // 2, offset=o)
    nib = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]
    qual = np.frombuffer(b, dtype=np.uint8, count=l_seq, offset=o + (l_seq + 1) // 2)
    return Read(ref, pos0, L, bool(c.flag & 0x10), nib.astype(np.int64), qual)


@dataclass
class Resolved:
    ref: np.ndarray        # int32, by refID then position
    pos0: np.ndarray       # uint32
    given: int             # sites after merging, resolved or not
    first: dict            # contig name -> its first refID
    start: dict            # refID -> (index of its first site, its positions as int64)


def resolve(sites, refs: list, contigs: dict) -> Resolved:
    """sites: iterable of (contig name, 0-based position); contigs: name -> length of the genome's contigs"""
    by_name = {}
    for n, p in sites:
        by_name.setdefault(n, set()).add(int(p))
    first = {}
    for i, (n, _) in enumerate(refs):
        first.setdefault(n, i)
    rr, pp, start, at = [], [], {}, 0
    for i, (n, _) in enumerate(refs):
        if first[n] != i or n not in contigs or n not in by_name:
            continue
        pos = np.array(sorted(p for p in by_name[n] if p < contigs[n]), dtype=np.int64)
        start[i] = (at, pos)
        rr.append(np.full(pos.size, i, dtype=np.int32))
        pp.append(pos.astype(np.uint32))
        at += pos.size
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)  # noqa: E731
    return Resolved(cat(rr, np.int32), cat(pp, np.uint32), sum(len(v) for v in by_name.values()), first, start)


def count(reads, res: Resolved, refs: list, trim: int = 0, min_bq: int = 0) -> np.ndarray:
    """counts[n, 10] uint32 of the reads (Read) at the resolved sites"""
    counts = np.zeros((res.ref.size, 10), dtype=np.int64)
    for r in reads:
        slot = res.start.get(res.first[refs[r.ref][0]])
        if slot is None or 2 * trim >= r.L:
            continue
        at, pos = slot
        k0, k1 = np.searchsorted(pos, [r.pos0 + trim, r.pos0 + r.L - trim])
        if k0 == k1:
            continue
        off = pos[k0:k1] - r.pos0
        inside = off < r.nib.size
        code = np.full(off.size, 4, dtype=np.int64)
        code[inside] = CODE_OF_NIBBLE[r.nib[off[inside]]]
        if min_bq:
            low = np.zeros(off.size, dtype=bool)
            low[inside] = r.qual[off[inside]] < min_bq
            code[low] = 4
        np.add.at(counts, (at + np.arange(k0, k1), code + (5 if r.rev else 0)), 1)
    return counts.astype(np.uint32)


def count_brute(reads, res: Resolved, refs: list, trim: int = 0, min_bq: int = 0) -> np.ndarray:
    """the same, read by read and base by base through a dictionary of the sites"""
    where = {(int(r), int(p)): j for j, (r, p) in enumerate(zip(res.ref, res.pos0))}
    counts = np.zeros((res.ref.size, 10), dtype=np.uint32)
    for r in reads:
        ref = res.first[refs[r.ref][0]]
        for off in range(trim, r.L - trim):
            j = where.get((ref, r.pos0 + off))
            if j is None:
                continue
            n = int(r.nib[off]) if off < r.nib.size else 0
            code = {1: 0, 2: 1, 4: 2, 8: 3}.get(n, 4)
            if min_bq and off < r.qual.size and r.qual[off] < min_bq:
                code = 4
            counts[j, code + (5 if r.rev else 0)] += 1
    return counts


def ref_bases(res: Resolved, refs: list, seqs: dict) -> np.ndarray:
    """the genome's letter at every resolved site (seqs: contig name -> sequence): A C G T, anything else N"""
    return np.array([ord(c) if (c := seqs[refs[int(r)][0]][int(p)].upper()) in "ACGT" else ord("N") for r, p in zip(res.ref, res.pos0)], dtype=np.uint8)


def totals(res: Resolved, counts: np.ndarray) -> dict:
    sums = counts.astype(np.int64).sum(axis=1)
    return {"given": res.given, "resolved": int(res.ref.size), "covered": int((sums > 0).sum()), "bases": int(sums.sum())}


def from_raw(raw_kept, refs: list, contigs: dict, sites, trim: int = 0, min_bq: int = 0):
    """-> (Resolved, counts) of the kept records at the sites"""
    res = resolve(sites, refs, contigs)
    return res, count([read_of_raw(b) for b in dl.split_raw(raw_kept)], res, refs, trim, min_bq)


# ---- the sites file and the report ---------------------------------------------------------------------------------------------------

def parse_sites(text: str) -> list:
    """[(contig, 0-based position)] of a sites file; ValueError("line N: ...") for a line host/alleles.c refuses"""
    out = []
    for no, line in enumerate(text.split("\n"), 1):
        line = line[:-1] if line.endswith("\r") else line
        line = line.lstrip(" \t")
        if not line or line.startswith("#"):
            continue
        f = line.replace("\t", " ").split()
        if len(f) < 2:
            raise ValueError(f"line {no}: a site needs two fields")
        if not (f[1].isascii() and f[1].isdigit()):
            raise ValueError(f"line {no}: the position is not a decimal integer")
        if not 1 <= int(f[1]) <= 2 ** 32:
            raise ValueError(f"line {no}: the position is 1-based and at most 2^32")
        out.append((f[0], int(f[1]) - 1))
    if not out:
        raise ValueError("the file holds no site")
    return out


def sites_text(sites) -> str:
    return "".join(f"{n}\t{p + 1}\n" for n, p in sites)


def report_text(fasta: str, bam: str, sites_fn: str, trim: int, refs: list, res: Resolved, bases: np.ndarray, counts: np.ndarray) -> str:
    t = totals(res, counts)
    lines = [f"# pss-bam allele counts  fasta {fasta} bam {bam} sites {sites_fn}  trim {trim}",
             f"# sites_given {t['given']} sites_resolved {t['resolved']} sites_covered {t['covered']} bases_counted {t['bases']}",
             "#contig\tpos\tref\t" + "\t".join(COLUMNS)]
    for r, p, b, c in zip(res.ref, res.pos0, bases, counts):
        lines.append(f"{refs[int(r)][0]}\t{int(p) + 1}\t{chr(int(b))}\t" + "\t".join(str(int(v)) for v in c))
    return "\n".join(lines) + "\n"


def report_of_raw(fasta, bam, sites_fn, trim, refs, seqs: dict, raw_kept, sites, min_bq: int = 0) -> str:
    res, counts = from_raw(raw_kept, refs, {n: len(s) for n, s in seqs.items()}, sites, trim, min_bq)
    return report_text(str(fasta), str(bam), str(sites_fn), trim, refs, res, ref_bases(res, refs, seqs), counts)


# ---- the golden ----------------------------------------------------------------------------------------------------------------------

def golden_reads():
    """(refs, seqs, reads) behind tests/golden/alleles_setD.txt: the record set of the coverage golden (coverage_lib.kept_of_golden),
    as records"""
    refs, raw = tl.read_bam(GOLD / "setD.bam")
    seqs = dict(dl.read_fasta(GOLD / "setD.fa"))
    s = dl.Setup(refs, {n: len(q) for n, q in seqs.items()}, pss=tl.PssOpts())
    kept = [read_of_raw(b) for b in dl.split_raw(raw) if cl.kept(cl.core_of_raw(b), s)]
    return refs, seqs, kept + kept[::5] + kept[::5]


def golden_sites(refs, seqs) -> list:
    """every 37th position of every contig of setD, one contig the genome lacks and one position beyond a contig's end"""
    out = [(n, p) for n, q in seqs.items() for p in range(3, len(q), 37)]
    name = next(iter(seqs))
    return out + [("no_such_contig", 10), (name, len(seqs[name]) + 5), out[0]]


def golden_text() -> tuple:
    """(the sites file, the report) of the golden"""
    refs, seqs, reads = golden_reads()
    sites = golden_sites(refs, seqs)
    res = resolve(sites, refs, {n: len(q) for n, q in seqs.items()})
    counts = count(reads, res, refs, trim=0)
    return sites_text(sites), report_text("setD.fa", "setD.bam", "alleles_setD.sites", 0, refs, res, ref_bases(res, refs, seqs), counts)

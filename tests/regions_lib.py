"""The yardstick of pss-bam -T / fragkon -T, shared by test_regions_host.py and test_gpu_regions.py.

`-T regions.bed` on a file == the tool without -T on the same file reduced to the records `samtools view -L
regions.bed` keeps: a record is kept when [POS-1, POS-1 + reference length of its CIGAR) meets an interval [start, end)
of its own contig.  keep_rec is that rule in plain Python, reduce_recs / write_reduced_sam build the second file, and
fuzz_intervals makes interval sets for a pssbam_testlib.fuzz_dataset that hit the edges of the rule and of the engine's
lookup table on purpose.  direct_keep is an independent restatement (a per-base coverage mask and the length the tools'
own filters use) against which keep_rec is checked once, on the CPU oracle."""
from __future__ import annotations

from pathlib import Path

import numpy as np

import pssbam_testlib as tl

# the seeds the GPU tests use; test_regions_host.py asserts on the CPU oracle that each keeps and drops >= 10 % of the
# records the unfiltered run tallies
PSS_SEEDS = (9301, 9302)
FK_SEEDS = (9311,)
RG_SEEDS = (9321,)      # fuzz_dataset(with_rg=True): -R, -G and the command-line tests
N_READS = 1500


def fuzz_case(seed: int):
    """(contigs, refs, recs, intervals) of one seed"""
    contigs, refs, recs = tl.fuzz_dataset(seed, N_READS, with_rg=seed in RG_SEEDS)
    return contigs, refs, recs, fuzz_intervals(seed, contigs, recs)


# more than 64 references (shapes of test_gpu_many_refs.py / test_gpu_contig_sets.py): regions only on contigs whose
# refID is 64 or above, and regions that include a contig literally named "*"
MANY_REFS_SEED, STAR_SEED = 9331, 9332
MANY_REFS_IVS = [("tiny.6", 0, 1200), ("tiny.5", 100, 400), ("tiny.4", 300, 600), ("tiny.4", 590, 640), ("scaffold_10", 299, 300)]
STAR_IVS = [("*", 0, 1500), ("chrB", 1000, 3000), ("chrA", 0, 1200), ("unplaced_100", 0, 50), ("tiny.6", 2400, 2600)]


def regions_dict(ivs) -> dict:
    """[(name, start, end)] -> {name: [(start, end)]} without the empty intervals"""
    out: dict = {}
    for nm, s, e in ivs:
        out.setdefault(nm, [])
        if s < e:
            out[nm].append((s, e))
    return out


def keep_rec(rec: tl.Rec, regions: dict) -> bool:
    """the `samtools view -L` rule: the alignment [POS-1, POS-1 + reference length), the length 1 when the CIGAR
    consumes no reference base, shares a base with an interval of the record's contig"""
    span = rec.ref_span() or 1
    a, b = rec.pos - 1, rec.pos - 1 + span
    return any(s < b and a < e for s, e in regions.get(rec.rname, ()))


def reduce_recs(recs: list, ivs) -> list:
    reg = regions_dict(ivs)
    return [r for r in recs if keep_rec(r, reg)]


def write_reduced_sam(path: Path, refs, recs, ivs) -> list:
    kept = reduce_recs(recs, ivs)
    tl.write_sam(path, refs, kept)
    return kept


def coverage(ivs, size: int = 1 << 14) -> dict:
    """{name: bool array, True where a base lies in some interval}"""
    cov: dict = {}
    for nm, s, e in ivs:
        m = cov.setdefault(nm, np.zeros(size, dtype=bool))
        m[min(s, size):min(e, size)] = True
    return cov


def direct_keep(rec: tl.Rec, cov: dict, kmer: bool = False) -> bool:
    """for records either tool can tally (CIGAR exactly <L>M): does a base of [s, s + L) lie in a region?  L is the
    length the tool's own filters compare with the CIGAR (pss: |TLEN| when paired, else strlen(SEQ); fragkon: strlen(SEQ))"""
    L = len(rec.seq) if kmer or not (rec.flag & 1) else abs(rec.tlen)
    m = cov.get(rec.rname)
    s = rec.pos - 1
    return m is not None and s >= 0 and bool(m[s:s + L].any())


def to_arrays(ivs):
    """-> (names, name_of, starts, ends) as Engine.set_regions takes them"""
    names: list[str] = []
    for nm, _, _ in ivs:
        if nm not in names:
            names.append(nm)
    return (names, np.array([names.index(nm) for nm, _, _ in ivs], dtype=np.int32),
            np.array([s for _, s, _ in ivs], dtype=np.uint32), np.array([e for _, _, e in ivs], dtype=np.uint32))


def write_bed(path: Path, ivs, messy: bool = True) -> None:
    """BED text; `messy`: a track line, a browser line, a comment, an empty line, blanks as separators, extra fields"""
    out = ["track name=targets\n", "browser position chrB:1-100\n", "# a comment\n", "\n"] if messy else []
    for k, (nm, s, e) in enumerate(ivs):
        out.append(f"{nm} {s}  {e}\n" if messy and k % 5 == 3 else f"{nm}\t{s}\t{e}\tiv{k}\t0\t+\n" if messy and k % 5 == 1
                   else f"{nm}\t{s}\t{e}\n")
    path.write_text("".join(out))


def fuzz_intervals(seed: int, contigs, recs) -> list:
    """Intervals [(name, start, end)] for a fuzz_dataset with contigs chrB (5000), chrA (1200) and scaffold_10 (300):
    on chrB intervals that start exactly at a read's end and end exactly at a read's start (touching, not overlapping),
    overlaps of exactly one base on each side, nested + overlapping + adjacent intervals (they merge), an empty
    interval, 20 one-base intervals inside one 1024-base grid bin, an interval spanning twelve 16-base bins, an
    interval at base 0 and one running past the contig end; random ones on chrA (one past its end); none on
    scaffold_10; a name that is in no header and one that is in the header only.  Deliberately out of order."""
    rng = np.random.default_rng(seed)
    lens = {nm: len(s) for nm, s in contigs}
    assert lens["chrB"] >= 5000 and lens["chrA"] >= 1200 and "scaffold_10" in lens
    ivs = [("chrB", 0, 40), ("chrB", 4900, 6000), ("chrB", 3500, 3500),
           ("chrB", 3000, 3200), ("chrB", 3050, 3100), ("chrB", 3150, 3300), ("chrB", 3300, 3350)]
    ivs += [("chrB", 3600 + 2 * k, 3601 + 2 * k) for k in range(20)]
    # around the alignments of plain <L>M reads in the quiet part of chrB
    plain = [r for r in recs if r.rname == "chrB" and len(r.cigar) == 1 and r.cigar[0][1] == "M" and 300 <= r.pos - 1
             and r.pos - 1 + r.cigar[0][0] <= 2800 and r.cigar[0][0] >= 20]
    pick = [plain[int(i)] for i in rng.choice(len(plain), size=8, replace=False)]
    for k, r in enumerate(pick):
        s, e = r.pos - 1, r.pos - 1 + r.cigar[0][0]
        ivs.append([("chrB", e, e + 7), ("chrB", s - 5, s), ("chrB", e - 1, e + 3), ("chrB", s - 3, s + 1)][k % 4])
    for _ in range(int(rng.integers(4, 9))):
        s = int(rng.integers(0, 1150))
        ivs.append(("chrA", s, s + int(rng.integers(1, 120))))
    ivs += [("chrA", 1180, 1300), ("chrNowhere", 0, 1000), ("chrMissing", 0, 4000)]
    order = rng.permutation(len(ivs))
    return [ivs[int(i)] for i in order]


def read_bed(path: Path) -> list:
    """a plain-text BED -> [(name, start, end)] (what the tools' reader accepts, without its error checks)"""
    ivs = []
    for ln in Path(path).read_text().splitlines():
        f = ln.split()
        if not f or ln.lstrip().startswith(("#", "track", "browser")):
            continue
        ivs.append((f[0], int(f[1]), int(f[2])))
    return ivs


def reduce_sam_text(text: str, ivs) -> str:
    """the same reduction on SAM text (header lines pass through)"""
    import re
    reg = regions_dict(ivs)
    out = []
    for ln in text.splitlines(keepends=True):
        if not ln.startswith("@"):
            f = ln.split("\t")
            span = sum(int(n) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5]) if op in "MDN=X") or 1
            a = int(f[3]) - 1
            if not any(s < a + span and a < e for s, e in reg.get(f[2], ())):
                continue
        out.append(ln)
    return "".join(out)

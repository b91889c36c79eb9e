#!/usr/bin/env python3
"""Writes the damaged fixture of pss-bam -E and its expected files:

    tests/golden/setD.fa / setD.sam / setD.bam     a seeded library: three A/C/G/T contigs of about 2 kb, at most 700
                                                   reads of 15..80 bases on both strands, about a fifth of them paired,
                                                   terminal C->T / G->A damage at a rate that falls off inward, a few
                                                   reads with low-quality terminal bases
    tests/golden/cond_<case>_setD.pss.{counts,rates,reads}.txt   for the cases ss, ds, ss3 (-E ss,3) and ss_q20 (-E ss -Q 20)

The expected files come from the unmodified reference (oracle/_ref/pss-bam, its default options) on setD.sam reduced by
end_condition_lib.reduce_sam_text: the forward section is the one it writes for the unpaired 3'-marked records, the
reverse section the one for the 5'-marked records, and the read counts are row -2 of its forward table on each
reduction (every contig is pure A/C/G/T, so each tallied unpaired read adds one there).  -Q 20 is the reference on the
reduction with every base below Q20 set to N.  Needs oracle/_ref, which only a machine that holds the reference's
sources can build; run from anywhere:

    python tests/golden/make_end_condition_golden.py
"""
import os
import shutil
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import base_quality_lib as bq        # noqa: E402
import end_condition_lib as ec       # noqa: E402
import pssbam_testlib as tl          # noqa: E402

SEED = 20261
CASES = {"ss": (1, 13, 13, 0), "ds": (1, 13, 2, 0), "ss3": (3, 13, 13, 0), "ss_q20": (1, 13, 13, 20)}   # depth, cell5, cell3, -Q
READ_NAMES = ("unpaired_reads", "marked_5p", "marked_3p", "marked_both")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def library():
    rng = np.random.default_rng(SEED)
    contigs = [(f"ctg{k + 1}", "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=int(ln)))) for k, ln in enumerate((2100, 1900, 2000))]
    recs = []
    for i in range(690):
        name, ref = contigs[int(rng.integers(0, 3))]
        L = int(rng.integers(15, 81))
        s = int(rng.integers(2, len(ref) - L - 2))
        is_rev = bool(rng.random() < 0.5)
        # read orientation: o copies g but for damage; 5' C->T, 3' C->T (single-stranded protocols) or G->A (double-stranded)
        g = ref[s:s + L] if not is_rev else "".join(COMP[c] for c in reversed(ref[s:s + L]))
        o = list(g)
        for k in range(min(6, L)):
            p = 0.85 / (1 + k) ** 1.3
            if g[k] == "C" and rng.random() < p:
                o[k] = "T"
            if g[L - 1 - k] == "C" and rng.random() < p:
                o[L - 1 - k] = "T"
            if g[L - 1 - k] == "G" and rng.random() < p:
                o[L - 1 - k] = "A"
        for k in range(L):
            if rng.random() < 0.01:
                o[k] = "ACGTN"[int(rng.integers(0, 5))]
        q = [int(x) for x in rng.integers(25, 41, size=L)]
        if rng.random() < 0.12:             # low-quality terminal bases
            for k in range(int(rng.integers(1, 4))):
                q[k] = int(rng.integers(2, 20))
                q[L - 1 - k] = int(rng.integers(2, 20))
        seq, qual = "".join(o), "".join(chr(33 + x) for x in q)
        if is_rev:
            seq, qual = "".join(COMP.get(c, c) for c in reversed(seq)), qual[::-1]
        flag, tlen = (16 if is_rev else 0), 0
        if rng.random() < 0.2:              # a proper pair's first or second read
            flag |= 0x1 | 0x2 | (0x40 if rng.random() < 0.5 else 0x80)
            tlen = L if not is_rev else -L
        recs.append(tl.Rec(f"d{i:04d}", flag, name, s + 1, int(rng.integers(20, 61)), [(L, "M")], tlen=tlen, seq=seq, qual=qual))
    return contigs, [(n, len(s)) for n, s in contigs], recs


def splice(fwd_text: str, rev_text: str, marker: str) -> str:
    """the forward section of one report and the reverse section of another"""
    a, b = fwd_text.index(marker), rev_text.index(marker)
    return fwd_text[:a] + rev_text[b:]


def main() -> None:
    tl.build_oracle()
    if not tl.have_ref():
        sys.exit("oracle/_ref/pss-bam is missing: the reference's sources are needed to write these files")
    contigs, refs, recs = library()
    with tempfile.TemporaryDirectory() as tmp:   # relative names: the files' headers carry them
        os.chdir(tmp)
        tl.write_fasta(Path("setD.fa"), contigs, descr=False)
        tl.write_sam(Path("setD.sam"), refs, recs)
        tl.write_bam(Path("setD.bam"), refs, recs, rng=np.random.default_rng(SEED))
        text = Path("setD.sam").read_text()
        for case, (d, c5, c3, q) in CASES.items():
            out, reads = {}, []
            for which in ("unpaired", "5", "3", "both"):
                red = ec.reduce_sam_text(text, contigs, d, c5, c3, which, q)
                sam = Path(f"setD.{case}.{which}.sam")
                sam.write_text(bq.mask_sam_text(red, q) if q else red)
                out[which] = tl.run_ref_pss(Path("setD.fa"), sam, Path(f"{case}_{which}"), tl.PssOpts())
                reads.append(int(out[which][0][0].sum()))
            if not q and d == 1:                 # what keeps the golden from being vacuous
                assert min(reads[1:]) >= 20, (case, reads)
            Path(HERE / f"cond_{case}_setD.pss.counts.txt").write_text(splice(out["3"][2], out["5"][2], "### Reverse read substitution counts"))
            Path(HERE / f"cond_{case}_setD.pss.rates.txt").write_text(splice(out["3"][3], out["5"][3], "### Reverse read substitution rates"))
            Path(HERE / f"cond_{case}_setD.pss.reads.txt").write_text("".join(f"{n}\t{v}\n" for n, v in zip(READ_NAMES, reads)))
            print(case, reads)
        for name in ("setD.fa", "setD.sam", "setD.bam"):
            shutil.copy(name, HERE / name)
        os.chdir(HERE)


if __name__ == "__main__":
    main()

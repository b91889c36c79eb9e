#!/usr/bin/env python3
"""Writes tests/golden/composition10_setA.txt and composition10_setD.txt: the rows of the unmodified reference
(oracle/_ref/pss-bam) that the composition table of width w = 10 is tied to (include/pssbam_hip.h, composition_lib):

  tie1  the diagonal cells of the context rows -1 / -2 of the forward table (c5) and 1 / 2 of the reverse table (c3) of a run
        with the default options: rows w-1 and w-2 of the two blocks;
  tie2  the same input with every SEQ replaced by A's, -r 10: per position row j < 10 and reference base, the column sum over
        the read bases: rows w+j;
  tie3  the unpaired <L>M records at least w bases from both contig edges and at least 15 long, with -U / -D sets that hold
        every letter of the FASTA: for j = 3 .. 10 the records are lengthened by j - 2 bases at the end in question
        (composition_lib.shifted) and the diagonal of context row -2 of the forward table (c5) or 2 of the reverse table (c3)
        is row -j.

Each line is "<tie> <block> <offset> <A> <C> <G> <T>", TAB-separated; only numbers the reference printed are kept.  The script
checks composition_lib's restatement against every one of them before it writes.  Needs oracle/_ref, which only a machine
that holds the reference's sources can build; run from anywhere:

    python tests/golden/make_composition_golden.py
"""
import os
import shutil
import sys
import tempfile
from dataclasses import replace
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import composition_lib as cl         # noqa: E402
import mismatch_lib as ml            # noqa: E402
import pssbam_testlib as tl          # noqa: E402
import site_context_lib as sc        # noqa: E402

WIDTH = 10
MIN_LEN = 15


def reference_rows(base: str) -> dict:
    contigs = sc.read_fasta(HERE / f"{base}.fa")
    refs, recs = ml.read_sam(HERE / f"{base}.sam")
    w = WIDTH
    ties: dict = {}
    with tempfile.TemporaryDirectory() as tmp:
        fa = Path(tmp) / f"{base}.fa"
        shutil.copy(HERE / f"{base}.fa", fa)
        os.chdir(tmp)

        def run(name, rs, o):
            sam = Path(f"{name}.sam")
            tl.write_sam(sam, refs, rs)
            return tl.run_ref_pss(fa, sam, Path(name), o)[:2]

        ties["tie1"] = cl.context_rows(*run("plain", recs, tl.PssOpts()))
        ties["tie2"] = cl.inside_rows(*run("all_a", cl.all_a(recs), replace(tl.PssOpts(), region_len=w)), w)
        wide = replace(tl.PssOpts(), up_ctx=cl.fasta_letters(contigs), down_ctx=cl.fasta_letters(contigs))
        far = cl.far_from_edges(recs, contigs, w, MIN_LEN)
        ties["tie3"] = {}
        for block in ("c5", "c3"):
            for j in range(3, w + 1):
                rows = cl.context_rows(*run(f"{block}_{j}", cl.shifted(far, j, block), wide))
                ties["tie3"][(block, -j)] = rows[(block, -2)]
        os.chdir(HERE)
    return ties


def restated_rows(base: str) -> dict:
    """the same rows from composition_lib's restatement of the definition"""
    contigs = sc.read_fasta(HERE / f"{base}.fa")
    _, recs = ml.read_sam(HERE / f"{base}.sam")
    w = WIDTH
    rows = lambda c5, c3, js: {(b, j): [int(x) for x in t[j + w, :4]] for b, t in (("c5", c5), ("c3", c3)) for j in js}   # noqa: E731
    wide = replace(tl.PssOpts(), up_ctx=cl.fasta_letters(contigs), down_ctx=cl.fasta_letters(contigs))
    return {"tie1": rows(*cl.composition(recs, contigs, w)[:2], (-1, -2)),
            "tie2": rows(*cl.composition(recs, contigs, w, replace(tl.PssOpts(), region_len=w))[:2], range(w)),
            "tie3": rows(*cl.composition(cl.far_from_edges(recs, contigs, w, MIN_LEN), contigs, w, wide)[:2], range(-w, -2))}


def main() -> None:
    tl.build_oracle()
    if not tl.have_ref():
        sys.exit("oracle/_ref/pss-bam is missing: the reference's sources are needed to write these files")
    for base in ("setA", "setD"):
        ties = reference_rows(base)
        want = restated_rows(base)
        for tie in ties:
            assert ties[tie] == want[tie], (base, tie, [(k, ties[tie][k], want[tie][k]) for k in ties[tie] if ties[tie][k] != want[tie][k]])
        text = cl.golden_text(WIDTH, ties)
        (HERE / f"composition{WIDTH}_{base}.txt").write_text(text)
        print(base, {t: len(v) for t, v in ties.items()}, {t: sum(sum(v) for v in r.values()) for t, r in ties.items()})


if __name__ == "__main__":
    main()

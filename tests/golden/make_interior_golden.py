#!/usr/bin/env python3
"""Writes tests/golden/interior15_setD.txt: the read-interior substitution table of setD.sam at margin d = 15, from the
unmodified reference (oracle/_ref/pss-bam).  setD.sam is split into its unpaired and its paired records; for every distinct
length x of either part the reference runs with `-l x -L x -r x-d` on that part, and the table is the sum of the forward rows
d .. x-d-1 of every run plus the reverse rows d .. x-d-1 of the paired runs (a read 2 enters only there; an unpaired read is
whole in the forward rows already) -- interior_lib.reduce_runs.  Lengths below 2d + 1 have no such row and are not run.
`table` and `bases` are the reference's; the reference prints no read counts, so `reads` (tallied records with a non-empty
interior) and `tallied` come from interior_lib's restatement, whose table this script checks against the reference's first.
setD meets the non-vacuity conditions of tests/test_interior_host.py at d = 15, so the fall-back margin 5 is not used.
Needs oracle/_ref, which only a machine that holds the reference's sources can build; run from anywhere:

    python tests/golden/make_interior_golden.py
"""
import os
import shutil
import sys
import tempfile
from dataclasses import replace
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import interior_lib as il            # noqa: E402
import mismatch_lib as ml            # noqa: E402
import pssbam_testlib as tl          # noqa: E402
import site_context_lib as sc        # noqa: E402

MARGIN = 15
BASE = "setD"


def main() -> None:
    tl.build_oracle()
    if not tl.have_ref():
        sys.exit("oracle/_ref/pss-bam is missing: the reference's sources are needed to write this file")
    contigs = sc.read_fasta(HERE / f"{BASE}.fa")
    refs, recs = ml.read_sam(HERE / f"{BASE}.sam")
    d = MARGIN
    runs = []
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(HERE / f"{BASE}.fa", Path(tmp) / f"{BASE}.fa")
        os.chdir(tmp)
        for tag, part in zip(("unpaired", "paired"), il.split_sam(recs)):
            sam = Path(f"{tag}.sam")
            tl.write_sam(sam, refs, part)
            out = {}
            for x in sorted({il.pss_length(r) for r in part}):
                if x >= 2 * d + 1:
                    fwd, rev = tl.run_ref_pss(Path(f"{BASE}.fa"), sam, Path(f"{tag}{x}"),
                                              replace(tl.PssOpts(), min_read_len=x, max_read_len=x, region_len=x - d))[:2]
                    out[x] = (fwd, rev)
            runs.append(out)
        os.chdir(HERE)
    table = il.reduce_runs(d, *runs)
    want, reads, tallied = il.interior(recs, contigs, d)
    assert np.array_equal(table, want), (table, want)
    (HERE / f"interior{d}_{BASE}.txt").write_text(il.golden_text(d, table, reads, tallied))
    print(il.golden_text(d, table, reads, tallied), f"{len(runs[0])} unpaired and {len(runs[1])} paired runs")


if __name__ == "__main__":
    main()

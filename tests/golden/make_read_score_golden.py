#!/usr/bin/env python3
"""Writes tests/golden/pmd3_setD.pss.{counts,rates}.txt and tests/golden/pmd0_setA.pss.{counts,rates}.txt: the unmodified
reference (oracle/_ref/pss-bam, its default options) on setD.sam without the records whose post-mortem-damage score is below
3 nats (768 units), and on setA.sam without those below 0 (read_score_lib.reduce_sam_text).  The weights come from the
committed tests/golden/pmd_weights.txt, so nothing here depends on a libm.
Needs oracle/_ref, which only a machine that holds the reference's sources can build; run from anywhere:

    python tests/golden/make_read_score_golden.py
"""
import os
import shutil
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pssbam_testlib as tl          # noqa: E402
import read_score_lib as rs          # noqa: E402
import site_context_lib as sc        # noqa: E402

CASES = (("pmd3_setD", "setD", 3 * 256), ("pmd0_setA", "setA", 0))


def main() -> None:
    tl.build_oracle()
    if not tl.have_ref():
        sys.exit("oracle/_ref/pss-bam is missing: the reference's sources are needed to write these files")
    W = rs.committed_pmd_weights()
    with tempfile.TemporaryDirectory() as tmp:   # relative names: the files' headers carry them
        for tag, base, min_score in CASES:
            shutil.copy(HERE / f"{base}.fa", Path(tmp) / f"{base}.fa")
        os.chdir(tmp)
        for tag, base, min_score in CASES:
            contigs = sc.read_fasta(HERE / f"{base}.fa")
            reduced = Path(f"{base}.{tag}.sam")
            reduced.write_text(rs.reduce_sam_text((HERE / f"{base}.sam").read_text(), contigs, W, min_score))
            tl.run_ref_pss(Path(f"{base}.fa"), reduced, Path(tag), tl.PssOpts())
            for kind in ("counts", "rates"):
                shutil.copy(f"{tag}.pss.{kind}.txt", HERE / f"{tag}.pss.{kind}.txt")
        os.chdir(HERE)


if __name__ == "__main__":
    main()

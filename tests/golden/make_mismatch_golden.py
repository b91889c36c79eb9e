#!/usr/bin/env python3
"""Writes tests/golden/mism1_setA.pss.{counts,rates}.txt and tests/golden/mismtv0_setD.pss.{counts,rates}.txt: the
unmodified reference (oracle/_ref/pss-bam, its default options) on setA.sam without the records that have more than one
mismatch, and on setD.sam without the records that have a transversion (mismatch_lib.reduce_sam_text).
Needs oracle/_ref, which only a machine that holds the reference's sources can build; run from anywhere:

    python tests/golden/make_mismatch_golden.py
"""
import os
import shutil
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import mismatch_lib as ml            # noqa: E402
import pssbam_testlib as tl          # noqa: E402
import site_context_lib as sc        # noqa: E402

CASES = (("mism1_setA", "setA", 1, False), ("mismtv0_setD", "setD", 0, True))


def main() -> None:
    tl.build_oracle()
    if not tl.have_ref():
        sys.exit("oracle/_ref/pss-bam is missing: the reference's sources are needed to write these files")
    with tempfile.TemporaryDirectory() as tmp:   # relative names: the files' headers carry them
        for tag, base, k, tv_only in CASES:
            shutil.copy(HERE / f"{base}.fa", Path(tmp) / f"{base}.fa")
        os.chdir(tmp)
        for tag, base, k, tv_only in CASES:
            contigs = sc.read_fasta(HERE / f"{base}.fa")
            reduced = Path(f"{base}.{tag}.sam")
            reduced.write_text(ml.reduce_sam_text((HERE / f"{base}.sam").read_text(), contigs, k, tv_only))
            tl.run_ref_pss(Path(f"{base}.fa"), reduced, Path(tag), tl.PssOpts())
            for kind in ("counts", "rates"):
                shutil.copy(f"{tag}.pss.{kind}.txt", HERE / f"{tag}.pss.{kind}.txt")
        os.chdir(HERE)


if __name__ == "__main__":
    main()

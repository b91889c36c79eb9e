#!/usr/bin/env python3
"""Writes tests/golden/{cpg,noncpg}_setA.pss.{counts,rates}.txt: the unmodified reference (oracle/_ref/pss-bam, its
default options) on setA.sam with the read bases outside / inside CpG context set to N (site_context_lib.mask_sam_text).
Needs oracle/_ref, which only a machine that holds the reference's sources can build; run from anywhere:

    python tests/golden/make_site_context_golden.py
"""
import os
import shutil
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pssbam_testlib as tl          # noqa: E402
import site_context_lib as sc        # noqa: E402


def main() -> None:
    tl.build_oracle()
    if not tl.have_ref():
        sys.exit("oracle/_ref/pss-bam is missing: the reference's sources are needed to write these files")
    contigs = sc.read_fasta(HERE / "setA.fa")
    text = (HERE / "setA.sam").read_text()
    with tempfile.TemporaryDirectory() as tmp:   # relative names: the files' headers carry them
        shutil.copy(HERE / "setA.fa", Path(tmp) / "setA.fa")
        os.chdir(tmp)
        for tag, keep_in in (("cpg", True), ("noncpg", False)):
            masked = Path(f"setA.{tag}.sam")
            masked.write_text(sc.mask_sam_text(text, contigs, keep_in))
            tl.run_ref_pss(Path("setA.fa"), masked, Path(f"{tag}_setA"), tl.PssOpts())
            for kind in ("counts", "rates"):
                shutil.copy(f"{tag}_setA.pss.{kind}.txt", HERE / f"{tag}_setA.pss.{kind}.txt")
        os.chdir(HERE)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/rep1of3_setA.pss.{counts,rates}.txt: the unmodified reference (oracle/_ref/pss-bam, its default
options) on setA.sam reduced to the records of read-name replicate 1 of 3 (replicates_lib.reduce_sam_text: 227 of the 679
records).  Needs oracle/_ref, which only a machine that holds the reference's sources can build; run from anywhere:

    python tests/golden/make_replicates_golden.py
"""
import os
import shutil
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pssbam_testlib as tl          # noqa: E402
import replicates_lib as rp          # noqa: E402

TAG, BASE, K, J, N_KEPT = "rep1of3_setA", "setA", 3, 1, 227


def main() -> None:
    tl.build_oracle()
    if not tl.have_ref():
        sys.exit("oracle/_ref/pss-bam is missing: the reference's sources are needed to write these files")
    with tempfile.TemporaryDirectory() as tmp:   # relative names: the files' headers carry them
        shutil.copy(HERE / f"{BASE}.fa", Path(tmp) / f"{BASE}.fa")
        os.chdir(tmp)
        reduced = Path(f"{BASE}.{TAG}.sam")
        reduced.write_text(rp.reduce_sam_text((HERE / f"{BASE}.sam").read_text(), K, J))
        assert sum(not ln.startswith("@") for ln in reduced.read_text().splitlines()) == N_KEPT
        fwd, _, _, _, _ = tl.run_ref_pss(Path(f"{BASE}.fa"), reduced, Path(TAG), tl.PssOpts())
        assert fwd[2:].sum() > 0, "the reduction's forward table holds no count: pick another replicate"
        for kind in ("counts", "rates"):
            shutil.copy(f"{TAG}.pss.{kind}.txt", HERE / f"{TAG}.pss.{kind}.txt")
        os.chdir(HERE)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/alleles_setD.sites and tests/golden/alleles_setD.txt: a sites file and the report of `pss-bam -a` for it as the
Python restatement of the definition (tests/alleles_lib.py) gives it for the record set of the coverage golden
(coverage_lib.kept_of_golden: the records of setD.bam that pss-bam's default options keep by the candidate test, every fifth of them
three times over), trim 0, named as "setD.fa" / "setD.bam" / "alleles_setD.sites".  Needs nothing but the committed files; run from
anywhere:

    python tests/golden/make_alleles_golden.py
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import alleles_lib as al          # noqa: E402


def main() -> None:
    sites, report = al.golden_text()
    (HERE / "alleles_setD.sites").write_text(sites)
    (HERE / "alleles_setD.txt").write_text(report)


if __name__ == "__main__":
    main()

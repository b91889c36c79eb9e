#!/usr/bin/env python3
"""Writes tests/golden/duplicates_setD.txt: the report of `pss-bam -d` (<prefix>.pss.duplicates.txt) as the Python restatement of
the definition (tests/duplicates_lib.py) gives it for setD.bam's records followed by every third and then every fifth of them
once more (duplicates_lib.golden_input), under pss-bam's default options, named as "setD.fa" / "setD.dup.bam".
Needs nothing but the committed files; run from anywhere:

    python tests/golden/make_duplicates_golden.py
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import duplicates_lib as dl          # noqa: E402


def main() -> None:
    setup, raw = dl.golden_input()
    v = dl.judge_raw(raw, setup)
    (HERE / "duplicates_setD.txt").write_text(dl.report_text("setD.fa", "setD.dup.bam", v.totals, v.hist))


if __name__ == "__main__":
    main()

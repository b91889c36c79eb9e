#!/usr/bin/env python3
"""Writes tests/golden/coverage_setD.txt and tests/golden/coverage_setD.bedgraph: the files of `pss-bam -c -b` as the Python
restatement of the definition (tests/coverage_lib.py) gives them for the records of setD.bam that pss-bam's default options keep by
the candidate test, every fifth of them three times over (coverage_lib.kept_of_golden), named as "setD.fa" / "setD.bam".
Needs nothing but the committed files; run from anywhere:

    python tests/golden/make_coverage_golden.py
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import coverage_lib as cl          # noqa: E402


def main() -> None:
    refs, contigs, spans = cl.kept_of_golden()
    s = cl.from_spans(spans, refs, contigs)
    (HERE / "coverage_setD.txt").write_text(cl.coverage_text("setD.fa", "setD.bam", refs, contigs, s))
    (HERE / "coverage_setD.bedgraph").write_text(cl.bedgraph_text(refs, s.runs))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/rescale_setD.rates.txt: the rates file of `pss-bam -q 20` on setD, from an independent count of its tables
(tests/rescale_lib.py golden()), as the input of the quality-rescale tests.  Needs nothing but the committed files; run from anywhere:

    python tests/golden/make_rescale_golden.py
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import rescale_lib as rl          # noqa: E402


def main() -> None:
    g = rl.golden()
    assert g["kept"] != g["plain"] and len(g["kept"]) == len(g["plain"]) and g["built"]["near_half"] == 0
    (HERE / "rescale_setD.rates.txt").write_text(g["rates"])


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Writes tests/golden/windows_setD.windows.txt and tests/golden/windows_setD.gcbias.txt: the files of `pss-bam -w 64` as the Python
restatement of the definition (tests/windows_lib.py) gives them for the records behind coverage_setD.* (coverage_lib.kept_of_golden),
named as "setD.fa" / "setD.bam".  W = 64 (windows_lib.GOLDEN_W; the contigs have 2100, 1900 and 2000 bases): checked below to give setD full and short windows, windows that
are left out of the GC-bias table, and at least three non-empty GC bins.  Needs nothing but the committed files; run from anywhere:

    python tests/golden/make_windows_golden.py
"""
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import windows_lib as wl           # noqa: E402


def main() -> None:
    refs, seqs, spans = wl.golden()
    W = wl.GOLDEN_W
    win = wl.from_spans(spans, refs, seqs, W)
    size = win[2].astype(int) - win[1].astype(int)
    bw, _, used = wl.gcbias_rows(W, win)
    assert (size == W).any() and (size < W).any() and 0 < used < len(size) and sum(1 for n in bw if n) >= 3, (used, bw)
    assert int(win[6].sum()) > 0 and (win[5] > 0).any()
    (HERE / "windows_setD.windows.txt").write_text(wl.windows_text("setD.fa", "setD.bam", refs, W, win))
    (HERE / "windows_setD.gcbias.txt").write_text(wl.gcbias_text("setD.fa", "setD.bam", W, win))


if __name__ == "__main__":
    main()

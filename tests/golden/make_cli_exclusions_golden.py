#!/usr/bin/env python3
"""Writes tests/golden/cli_exclusions.txt: what a given build of pss-bam prints, and nothing else, for every command line of
tests/cli_exclusions_lib.py -- all ordered pairs of exclusive options and the lines beside them.  The file in the repository
was recorded from the build of the commit BEFORE the command's checks were folded into one table; record it from a build
that is known to be right, never from the one under test:

    python tests/golden/make_cli_exclusions_golden.py <path to bin/pss-bam>
"""
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import cli_exclusions_lib as xl   # noqa: E402


def main() -> None:
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    exe = Path(sys.argv[1]).resolve()
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for args in xl.cases():
            pr = xl.run(exe, args, Path(tmp))
            assert pr.returncode == 1 and pr.stdout == "" and not list(Path(tmp).iterdir()), (args, pr.returncode, pr.stdout)
            results.append((args, pr.stderr))
    (HERE / "cli_exclusions.txt").write_text(xl.golden_text(results))
    print(len(results), "command lines")


if __name__ == "__main__":
    main()

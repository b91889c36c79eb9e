"""pss-bam's check of the exclusive options, without a GPU: for every ordered pair of them (and the lines beside that check)
the command prints exactly the one line the build before the one-table check printed -- recorded in
tests/golden/cli_exclusions.txt by tests/golden/make_cli_exclusions_golden.py -- exits 1, and writes nothing.  And the sources
hold the rule once: the counts at the end are those the ladders could not meet."""
import re
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

import __graft_entry__ as ge
import cli_exclusions_lib as xl

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "cli_exclusions.txt"


@pytest.fixture(scope="module")
def pkg():
    ge.build()
    return ge.load_pkg()


def test_every_pair_prints_the_recorded_line_and_nothing_else(pkg, tmp_path):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    want = xl.read_golden(GOLDEN)
    cases = xl.cases()
    assert len(cases) == 309 and sorted(want) == sorted(" ".join(c) for c in cases)   # the enumeration is the recorded one
    with ThreadPoolExecutor(8) as pool:   # ~300 processes of a few ms each
        runs = list(pool.map(lambda args: xl.run(exe, args, tmp_path), cases))
    bad = [(args, pr.returncode, pr.stdout, pr.stderr, want[" ".join(args)]) for args, pr in zip(cases, runs)
           if pr.returncode != 1 or pr.stdout != "" or pr.stderr != want[" ".join(args)]]
    assert not bad, bad[:5]
    assert list(tmp_path.iterdir()) == []


def test_the_recorded_lines_follow_the_stated_rule():
    """the fixture itself: of two exclusive options the one later in the table is named first, in either argument order, the
    earlier one by its single-option label; -R, -Q and -T go with every one of them"""
    want = xl.read_golden(GOLDEN)
    label = {"-G": "-G (tables per read group)", "-S": "-S (tables per length bin)", "-C": "-C (tables per contig set)",
             "-H": "-H (fragment-length histogram)", "-X": "-X (tables per site context)", "-E": "-E (tables conditional on the other end)",
             "-I": "-I (clipped and gapped reads by their anchored ends)", "-A": "-A (tables per contig)", "-n": "-n (mismatch filter)",
             "-N": "-N (mismatch histogram)", "-V": "-V (count only transversions)", "-J": "-J (jackknife replicates)",
             "-W": "-W (read-interior table)", "-P": "-P (base composition around the read ends)", "-y": "-y (damage-score filter)",
             "-Y": "-Y (damage-score histogram)", "-n -N": "-n / -N (mismatch filter and histogram)",
             "-y -Y": "-y / -Y (damage-score filter and histogram)"}
    name = lambda args: " ".join(a for a in args if a.startswith("-"))   # noqa: E731
    order = [row for _, row in xl.SPELLINGS[:16]]
    needs = "-V (count only transversions) needs -n (mismatch filter) or -N (mismatch histogram).\n"
    for a, row_a in xl.SPELLINGS:
        for b, row_b in xl.SPELLINGS:
            if row_a == row_b:
                continue
            got = want[" ".join(a + b)]
            (mine, _), (other, _) = sorted(((a, row_a), (b, row_b)), key=lambda x: order.index(x[1]))[::-1]
            if "-V" in (name(a), name(b)) and "-J" not in (name(a), name(b)):
                assert got == needs, (a, b, got)
            else:
                assert got == f"{label[name(mine)]} and {label[name(other)[:2]]} exclude each other.\n", (a, b, got)
    for a, _ in xl.SPELLINGS:
        got = want[" ".join(a + xl.GOES_WITH)]
        if name(a) == "-G":
            assert got == "-G (tables per read group) and -R (one read group) exclude each other.\n"
        elif name(a) == "-V":
            assert got == needs
        else:
            assert got == "-T: unable to read the BED file (no.bed)\n", (a, got)
    assert want["-E bad -G"].startswith("-E (tables conditional on the other end): unknown preset")
    assert want["-H bad -G"] == "-H (fragment-length histogram) and -G (tables per read group) exclude each other.\n"


def test_the_rule_is_written_once_per_module():
    host = ROOT / "pss-bam_amd" / "host"
    engine = (ROOT / "pss-bam_amd" / "csrc" / "engine.hip").read_text()
    main_c = (host / "pss_main.c").read_text()
    code = main_c[main_c.index("*/", main_c.index("pss_main.c")) :]   # (the header comment is documentation)
    assert engine.count("exclude each other") <= 2 and code.count("exclude each other") <= 2
    for lab in ("-G (tables per read group)", "-S (tables per length bin)", "-C (tables per contig set)", "-H (fragment-length histogram)",
                "-X (tables per site context)", "-E (tables conditional on the other end)", "-I (clipped and gapped reads by their anchored ends)",
                "-A (tables per contig)", "-n (mismatch filter)", "-N (mismatch histogram)", "-V (count only transversions)",
                "-J (jackknife replicates)", "-W (read-interior table)", "-P (base composition around the read ends)",
                "-y (damage-score filter)", "-Y (damage-score histogram)", "-n / -N (mismatch filter and histogram)",
                "-y / -Y (damage-score filter and histogram)"):
        assert code.count(lab) == 1, lab
    assert (host / "frontend.c").read_text().count("pssbam_engine_set_length_histogram(") == 1
    assert len(re.findall(r"^extern .*frontend_", (host / "frontend.h").read_text(), re.M)) == 2

"""The command lines on which pss-bam's check of the exclusive options is recorded and tested: what
tests/golden/make_cli_exclusions_golden.py runs to write tests/golden/cli_exclusions.txt and what
tests/test_cli_exclusions_host.py runs against it.  Every command names a FASTA, a BAM, a map and a BED file that do not
exist, by relative names, so it ends before any work and its one line on stderr holds no path of the machine."""
import subprocess
from pathlib import Path

# one spelling per exclusive option, in the order of the command's table; the rows of -n / -N / -V and of -y / -Y hold several
SPELLINGS = [(["-G"], "G"), (["-S", "40"], "S"), (["-C", "nomap"], "C"), (["-H", "100"], "H"), (["-X", "cpg"], "X"), (["-E", "ss"], "E"),
             (["-I"], "I"), (["-A"], "A"), (["-n", "1"], "mism"), (["-N", "4"], "mism"), (["-V"], "mism"), (["-J", "8"], "J"),
             (["-W", "5"], "W"), (["-P", "5"], "P"), (["-y", "1"], "score"), (["-Y"], "score"),
             (["-n", "1", "-N", "4"], "mism"), (["-y", "1", "-Y"], "score")]
GOES_WITH = ["-R", "g", "-Q", "20", "-T", "no.bed"]


def cases() -> list[list[str]]:
    """every ordered pair of spellings from different rows; the one-sided -G / -R rule, -E's value (parsed before the check) and
    -H's (parsed after it); and every spelling beside -R, -Q and -T"""
    out = [a + b for a, row_a in SPELLINGS for b, row_b in SPELLINGS if row_a != row_b]
    out += [["-G", "-R", "x"], ["-E", "bad", "-G"], ["-H", "bad", "-G"]]
    out += [a + GOES_WITH for a, _ in SPELLINGS]
    return out


def run(exe: Path, args: list[str], cwd: Path) -> subprocess.CompletedProcess:
    return subprocess.run([str(exe), "-F", "no.fa", "-B", "no.bam", "-o", "out", *args], cwd=cwd, capture_output=True, text=True, timeout=60)


def golden_text(results: list[tuple[list[str], str]]) -> str:
    """"$ <arguments>" and the bytes of stderr, in turn"""
    return "".join(f"$ {' '.join(args)}\n{err}" for args, err in results)


def read_golden(path: Path) -> dict[str, str]:
    want: dict[str, str] = {}
    key = None
    for line in path.read_text().splitlines(keepends=True):
        if line.startswith("$ "):
            key = line[2:-1]
            want[key] = ""
        else:
            want[key] += line
    return want

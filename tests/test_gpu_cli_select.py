"""pss-bam -O end to end on the GPU: the tables stay what they are, the BAM is complete the moment the command returns (also
under the detached exit), holds the input's header and exactly the tallied records, and is the file "the input without the
other reads" that the filters' descriptions speak of -- the unmodified reference on it, with default options, writes the
tables it writes for the whole input with the filter."""
import os
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
ROUTES = {"detached": {}, "one_process": {"PSSBAM_DETACH_EXIT": "0"}, "host_reader": {"PSSBAM_DEVICE_INFLATE": "0"}}


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert (p.PKG_DIR / "bin" / "pss-bam").exists(), "front ends not built (run __graft_entry__.build())"
    return p


def run_cli(pkg, fa, aln, prefix, *more, env=None):
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    return subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(prefix), *more], capture_output=True, text=True,
                          env={**os.environ, **(env or {})}, timeout=300)


def report_body(text: str) -> str:
    return "".join(ln for ln in text.splitlines(keepends=True) if not ln.startswith(("### FASTA", "### BAM", "### OUT")))


def header_bytes(raw: bytes) -> int:
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    return o


def records(raw: bytes, o: int) -> list:
    out = []
    while o < len(raw):
        n = 4 + struct.unpack_from("<I", raw, o)[0]
        out.append(raw[o:o + n])
        o += n
    assert o == len(raw)
    return out


CASES = {"q20_setA": ("setA", ["-q", "20"], None), "y3_setD": ("setD", ["-y", "3"], "pmd3_setD")}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", list(CASES))
def test_cli_O(pkg, oracle, tmp_path, case, route):
    base, args, golden = CASES[case]
    fa, aln, out = GOLD / f"{base}.fa", GOLD / f"{base}.bam", tmp_path / "out.bam"
    pr = run_cli(pkg, fa, aln, tmp_path / "out", *args, "-O", str(out), env=ROUTES[route])
    # complete the moment the command returns: read at once, before anything else runs
    data = out.read_bytes() if out.exists() else b""
    assert pr.returncode == 0, pr.stderr
    assert data[-28:] == tl.BGZF_EOF and not Path(str(out) + ".tmp").exists()
    assert pr.stderr.splitlines()[0].endswith(f" -O {out} -z 1")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.bam", "out.pss.counts.txt", "out.pss.rates.txt"]
    # the tables: those of the run without -O (and the golden, where the reference wrote one)
    plain = run_cli(pkg, fa, aln, tmp_path / "plain", *args, env=ROUTES[route])
    assert plain.returncode == 0, plain.stderr
    for kind in ("counts", "rates"):
        mine = report_body((tmp_path / f"out.pss.{kind}.txt").read_text())
        assert mine == report_body((tmp_path / f"plain.pss.{kind}.txt").read_text()), kind
        if golden:
            assert mine == report_body((GOLD / f"{golden}.pss.{kind}.txt").read_text()), kind
    # header and records: the input's header bytes, a subsequence of the input's records, as many as were tallied
    raw_in, raw_out = tl.bgzf_inflate(aln.read_bytes()), tl.bgzf_inflate(data)
    hb = header_bytes(raw_in)
    assert raw_out[:hb] == raw_in[:hb] and header_bytes(raw_out) == hb
    rin, rout = records(raw_in, hb), records(raw_out, hb)
    j = 0
    for b in rout:
        while j < len(rin) and rin[j] != b:
            j += 1
        assert j < len(rin), "a written record is not in the input, or out of order"
        j += 1
    stats = run_cli(pkg, fa, aln, tmp_path / "st", *args, env={**ROUTES[route], "PSSBAM_STATS": "1"})
    n_ok = int([ln for ln in stats.stderr.splitlines() if ln.startswith("[pssbam] pss_ok=")][0].split("=")[1])
    assert len(rout) == n_ok and 0 < n_ok < len(rin)
    # the README's equivalence: default options on out.bam == the filter on the input -- by this command ...
    again = run_cli(pkg, fa, out, tmp_path / "again", env=ROUTES[route])
    assert again.returncode == 0, again.stderr
    gf, gr = tl.parse_counts_text((tmp_path / "again.pss.counts.txt").read_text())
    wf, wr = tl.parse_counts_text((tmp_path / "out.pss.counts.txt").read_text())
    assert np.array_equal(gf, wf) and np.array_equal(gr, wr) and wf[2:].sum() > 0
    # ... and by the unmodified reference, against its own tables for the input with the filter (-q: its own option; -y: the
    # committed tables it wrote for the reduced input)
    if tl.have_ref():
        b2s = str(pkg.PKG_DIR / "bin" / "bam2sam")
        rf, rr, _, _, _ = tl.run_ref_pss(fa, out, tmp_path / "ref_out", tl.PssOpts(), bam2sam=b2s)
        if case == "q20_setA":
            xf, xr, _, _, _ = tl.run_ref_pss(fa, aln, tmp_path / "ref_in", tl.PssOpts(min_mq=20), bam2sam=b2s)
        else:
            xf, xr = tl.parse_counts_text((GOLD / f"{golden}.pss.counts.txt").read_text())
        assert np.array_equal(rf, xf) and np.array_equal(rr, xr) and np.array_equal(rf, wf) and np.array_equal(rr, wr)
    # a second pass over out.bam keeps every record: the file it writes is out.bam, byte for byte
    out2 = tmp_path / "out2.bam"
    second = run_cli(pkg, fa, out, tmp_path / "second", *args, "-O", str(out2), env=ROUTES[route])
    assert second.returncode == 0, second.stderr
    assert out2.read_bytes() == data


@pytest.mark.parametrize("level", ["0", "6"])
def test_cli_z(pkg, tmp_path, level):
    fa, aln = GOLD / "setD.fa", GOLD / "setD.bam"
    outs = {}
    for z in ("1", level):
        out = tmp_path / f"z{z}.bam"
        pr = run_cli(pkg, fa, aln, tmp_path / "out", "-m", "-O", str(out), "-z", z)
        assert pr.returncode == 0, pr.stderr
        outs[z] = out.read_bytes()
    assert tl.bgzf_inflate(outs["1"]) == tl.bgzf_inflate(outs[level]) and outs["1"] != outs[level]
    assert (len(outs[level]) > len(outs["1"])) == (level == "0")


@pytest.mark.parametrize("route", ["detached", "one_process"])
def test_a_failing_run_leaves_no_file(pkg, tmp_path, route):
    """the run tallies, writes out.bam.tmp and fails at the last step, the rename: -O names an existing directory.  Status 1, the
    writer's message, no temporary file, nothing in the directory, and no tables (the file is closed before they are written)"""
    out = tmp_path / "out.bam"
    out.mkdir()
    pr = run_cli(pkg, GOLD / "setA.fa", GOLD / "setA.bam", tmp_path / "out", "-q", "20", "-O", str(out), env=ROUTES[route])
    assert pr.returncode == 1, pr.stderr
    assert f"Error: -O: cannot rename {out}.tmp to {out}" in pr.stderr and "Full command" in pr.stderr and "Done." not in pr.stderr
    assert out.is_dir() and not list(out.iterdir()) and [p.name for p in tmp_path.iterdir()] == ["out.bam"]


def test_all_reads_filtered_gives_header_and_eof(pkg, tmp_path):
    out = tmp_path / "none.bam"
    pr = run_cli(pkg, GOLD / "setA.fa", GOLD / "setA.bam", tmp_path / "out", "-l", "100000", "-O", str(out))
    assert pr.returncode == 0, pr.stderr
    raw_in, raw = tl.bgzf_inflate((GOLD / "setA.bam").read_bytes()), tl.bgzf_inflate(out.read_bytes())
    assert raw == raw_in[:header_bytes(raw_in)] and out.read_bytes()[-28:] == tl.BGZF_EOF

"""The BAM writer (host/bam_writer.c: blocks cut by one thread, compressed by a pool, written in order) under ThreadSanitizer and
AddressSanitizer + UBSan, through the stand-alone drivers of `make -C pss-bam_amd sanitize`: `hostcheck.{tsan,asan} -a in.bam -w
out.bam` over a BAM of several batches of the writer must stay silent and write the plain build's file.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl

ENV = {"PSSBAM_BATCH_BYTES": "70000", "PSSBAM_INFLATE_THREADS": "4", "TSAN_OPTIONS": "halt_on_error=1 exitcode=66",
       "ASAN_OPTIONS": "detect_leaks=1 exitcode=67", "UBSAN_OPTIONS": "print_stacktrace=1 halt_on_error=1"}


@pytest.fixture(scope="module")
def san():
    ge.build()
    pkg = ge.load_pkg()
    pr = subprocess.run(["make", "-s", "-C", str(pkg.PKG_DIR), "sanitize"], capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr[-3000:]
    b = pkg.PKG_DIR / "bin"
    return b


@pytest.fixture(scope="module")
def big_bam(tmp_path_factory):
    """18 MB of records: more than one batch of 255 blocks, so the pool runs several rounds"""
    d = tmp_path_factory.mktemp("writer_san")
    contigs, refs, recs = tl.fuzz_dataset(4403, 2500, with_rg=True)
    raw = tl.bam_bytes(refs, recs)
    body = raw[len(tl.bam_bytes(refs, [])):]
    stream = raw + body * 39
    with open(d / "big.bam", "wb") as fh:
        for i in range(0, len(stream), 0xFF00):
            fh.write(tl.bgzf_block(stream[i:i + 0xFF00], 1))
        fh.write(tl.BGZF_EOF)
    assert len(stream) > 17 << 20
    return d / "big.bam"


def run(exe, src, dst, level, threads):
    pr = subprocess.run([str(exe), "-a", str(src), "-w", str(dst), "-z", str(level), "-t", str(threads)], capture_output=True, text=True,
                        timeout=900, env={**os.environ, **ENV})
    report = [ln for ln in pr.stderr.splitlines() if "Sanitizer" in ln or "runtime error" in ln]
    assert pr.returncode == 0 and not report, f"{exe.name}: rc {pr.returncode}\n" + pr.stderr[-3000:]
    return pr.stdout, dst.read_bytes()


@pytest.mark.parametrize("flavour", ["tsan", "asan"])
def test_writer_under_sanitizers(san, big_bam, tmp_path, flavour):
    if flavour == "tsan":   # (only this flavour depends on it)
        probe = subprocess.run([str(san / "san" / "hostcheck.tsan")], capture_output=True, text=True)
        if "unexpected memory mapping" in probe.stderr:
            pytest.skip("ThreadSanitizer cannot map its shadow in this environment")
    for level, threads in ((1, 8), (0, 3)):
        want_out, want = run(san / "hostcheck", big_bam, tmp_path / "plain.bam", level, threads)
        got_out, got = run(san / "san" / f"hostcheck.{flavour}", big_bam, tmp_path / "san.bam", level, threads)
        assert got_out == want_out and got == want and want[-28:] == tl.BGZF_EOF
    assert tl.bgzf_inflate(want) == tl.bgzf_inflate(big_bam.read_bytes())

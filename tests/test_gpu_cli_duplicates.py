"""pss-bam -d and fragkon -d end to end on the GPU: every file of a run with -d is byte for byte the file of the run without it on
the input whose duplicates -- as duplicates_lib, the Python restatement, names them -- carry FLAG 0x400, and the duplicates file is
the restatement's report.  Both runs of a pair see the same relative file names from a directory of their own, so the reports'
header lines agree too."""
import gzip
import os
import subprocess
from dataclasses import replace

import pytest

import __graft_entry__ as ge
import duplicates_lib as dl
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

PSS = tl.PssOpts(region_len=12, min_mq=20)
FK = tl.FkOpts(klen=5, min_mq=10)
GROUPS = ["grpA", "grpB"]


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert (p.PKG_DIR / "bin" / "pss-bam").exists(), "front ends not built (run __graft_entry__.build())"
    return p


@pytest.fixture(scope="module")
def data():
    contigs, refs, recs = tl.fuzz_dataset(6201, 600, with_rg=True)
    # every second copy goes to the other read group: under -G it is no duplicate of its original
    other = {"grpA": "grpB", "grpB": "grpA"}
    swap = lambda r: replace(r, tags=[(t, ty, other.get(v, v)) if (t, ty) == ("RG", "Z") else (t, ty, v) for t, ty, v in r.tags])  # noqa: E731
    return contigs, refs, [swap(r) if r.qname.endswith(".c1") else r for r in dl.with_copies(recs, 6201, max_copies=3)]


def stage(tmp_path, name, data, recs, sam=False):
    """a directory with g.fa and in.bam (or in.sam) of `recs`"""
    contigs, refs, _ = data
    d = tmp_path / name
    d.mkdir()
    tl.write_fasta(d / "g.fa", contigs)
    hdr = "@HD\tVN:1.6\tSO:unknown\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs) + "".join(f"@RG\tID:{g}\n" for g in GROUPS)
    if sam:
        (d / "in.sam").write_text(hdr + "".join(tl.sam_line(r) for r in recs))
    else:
        raw = tl.bam_bytes(refs, recs, text_header=hdr)
        (d / "in.bam").write_bytes(b"".join(tl.bgzf_block(raw[i:i + 0xFF00]) for i in range(0, len(raw), 0xFF00)) + tl.BGZF_EOF)
    return d


def cli(pkg, tool, d, *more, aln="in.bam", prefix=True):
    exe = pkg.PKG_DIR / "bin" / tool
    pr = subprocess.run([str(exe), "-F", "g.fa", "-B", aln, *(["-o", "p"] if prefix else []), *more], cwd=d, capture_output=True, text=True,
                        env=dict(os.environ), timeout=300)
    assert pr.returncode == 0, pr.stderr
    return pr


def outputs(d):
    return {p.name: p.read_bytes() for p in d.iterdir() if p.name.startswith("p.")}


def verdict(data, **setup):
    contigs, refs, recs = data
    return dl.judge_recs(recs, dl.Setup(refs, {n: len(s) for n, s in contigs}, **setup))


def test_pss_bam_d(pkg, data, tmp_path):
    v = verdict(data, pss=PSS)
    assert v.totals["flagged"] > 200
    a = stage(tmp_path, "a", data, data[2])
    b = stage(tmp_path, "b", data, dl.flag_recs(data[2], v.dup))
    pa = cli(pkg, "pss-bam", a, *PSS.argv(), "-d")
    cli(pkg, "pss-bam", b, *PSS.argv())
    assert pa.stderr.splitlines()[0].endswith(" -d")
    got, want = outputs(a), outputs(b)
    assert set(got) == set(want) | {"p.pss.duplicates.txt"} and set(want) == {"p.pss.counts.txt", "p.pss.rates.txt"}
    for k in want:
        assert got[k] == want[k], k
    assert got["p.pss.duplicates.txt"].decode() == dl.report_text("g.fa", "in.bam", v.totals, v.hist)
    cli(pkg, "pss-bam", stage(tmp_path, "c", data, data[2]), *PSS.argv())
    assert outputs(tmp_path / "c")["p.pss.counts.txt"] != got["p.pss.counts.txt"]      # (the setting does something)


def test_pss_bam_d_on_sam_text(pkg, data, tmp_path):
    v = verdict(data, pss=PSS)
    a = stage(tmp_path, "a", data, data[2], sam=True)
    b = stage(tmp_path, "b", data, dl.flag_recs(data[2], v.dup), sam=True)
    cli(pkg, "pss-bam", a, *PSS.argv(), "-d", aln="in.sam")
    cli(pkg, "pss-bam", b, *PSS.argv(), aln="in.sam")
    got, want = outputs(a), outputs(b)
    for k in want:
        assert got[k] == want[k], k
    assert got["p.pss.duplicates.txt"].decode() == dl.report_text("g.fa", "in.sam", v.totals, v.hist)


def test_pss_bam_d_O_Z_writes_the_deduplicated_bam(pkg, data, tmp_path):
    v = verdict(data, pss=PSS)
    a = stage(tmp_path, "a", data, data[2])
    b = stage(tmp_path, "b", data, dl.flag_recs(data[2], v.dup))
    cli(pkg, "pss-bam", a, *PSS.argv(), "-d", "-O", "kept.bam", "-Z")
    cli(pkg, "pss-bam", b, *PSS.argv(), "-O", "kept.bam", "-Z")
    got, want = gzip.decompress((a / "kept.bam").read_bytes()), gzip.decompress((b / "kept.bam").read_bytes())
    assert got == want and len(got) > 10000
    # kept records are never flagged: byte for byte the input's
    blobs = set(dl.split_raw(tl.raw_records(data[1], data[2])))
    kept = dl.split_raw(got[_header_bytes(got):])
    assert len(kept) > 100 and all(x in blobs for x in kept)


def _header_bytes(raw: bytes) -> int:
    import struct
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 4 + struct.unpack_from("<i", raw, o)[0] + 4
    return o


def test_pss_bam_d_G_writes_the_per_group_files(pkg, data, tmp_path):
    v = verdict(data, pss=PSS, groups=GROUPS)
    plain = verdict(data, pss=PSS)
    assert v.totals["distinct"] > plain.totals["distinct"]          # (the read group is part of the key)
    a = stage(tmp_path, "a", data, data[2])
    b = stage(tmp_path, "b", data, dl.flag_recs(data[2], v.dup))
    cli(pkg, "pss-bam", a, *PSS.argv(), "-d", "-G")
    cli(pkg, "pss-bam", b, *PSS.argv(), "-G")
    got, want = outputs(a), outputs(b)
    assert {"p.grpA.pss.counts.txt", "p.grpB.pss.rates.txt"} <= set(want) and set(got) == set(want) | {"p.pss.duplicates.txt"}
    for k in want:
        assert got[k] == want[k], k
    assert got["p.pss.duplicates.txt"].decode() == dl.report_text("g.fa", "in.bam", v.totals, v.hist)


def test_fragkon_d(pkg, data, tmp_path):
    v = verdict(data, fk=FK)
    assert v.totals["flagged"] > 200
    a = stage(tmp_path, "a", data, data[2])
    b = stage(tmp_path, "b", data, dl.flag_recs(data[2], v.dup))
    pa, pb = cli(pkg, "fragkon", a, *FK.argv(), "-d"), cli(pkg, "fragkon", b, *FK.argv())
    assert pa.stdout == pb.stdout and "p.fragkon.duplicates.txt" in outputs(a)
    assert outputs(a)["p.fragkon.duplicates.txt"].decode() == dl.report_text("g.fa", "in.bam", v.totals, v.hist)
    c = stage(tmp_path, "c", data, data[2])
    pc = cli(pkg, "fragkon", c, *FK.argv(), "-d", prefix=False)     # without -o: the table alone
    assert pc.stdout == pa.stdout and not outputs(c)
    assert cli(pkg, "fragkon", c, *FK.argv(), prefix=False).stdout != pa.stdout

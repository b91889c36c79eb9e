"""pss-bam -K without a GPU: the kernel's per-record function compiled for the host (tools/end_mask_emulate.cpp, a stand-alone
program under AddressSanitizer + UBSan over a heap block of exactly the stream's size), the same function on hostcheck's way to
the BAM writer, and what the command refuses.  The judge is end_mask_lib.mask_record, the definition restated on BAM bytes."""
import gzip
import subprocess
from pathlib import Path

import pytest

import __graft_entry__ as ge
import cli_exclusions_lib as xl
import end_mask_lib as em
import pssbam_testlib as tl

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("end_mask_emulate") / "end_mask_emulate"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "pss-bam_amd" / "csrc"),
                    "-o", str(out), str(ROOT / "tools" / "end_mask_emulate.cpp")], check=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def bins():
    ge.build()
    b = ge.load_pkg().PKG_DIR / "bin"
    assert (b / "hostcheck").exists() and (b / "pss-bam").exists() and (b / "fragkon").exists()
    return b


_STREAMS = {}


def stream(name: str) -> bytes:
    if name not in _STREAMS:
        _STREAMS[name] = em.crafted()[1].tobytes() if name == "crafted" else tl.read_bam(GOLD / f"{name}.bam")[1].tobytes()
    return _STREAMS[name]


def test_the_crafted_set_has_the_stated_properties():
    recs, raw, bad = em.crafted()
    blobs = em.split_records(raw)
    assert 200 < len(blobs) < 400
    lay = [em.layout(b) for b in blobs]
    assert {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33} <= {l for l, *_ in lay}
    assert [not fits for *_, fits in lay] == [i in bad for i in range(len(blobs))]
    first = {(rev, em.seq_qual(b)[0][0]) for b, (l, rev, _, _, fits) in zip(blobs, lay) if l and fits}
    last = {(rev, em.seq_qual(b)[0][-1]) for b, (l, rev, _, _, fits) in zip(blobs, lay) if l and fits}
    assert first >= {(rev, ch) for rev in (False, True) for ch in "ACGTN"} and last >= {(rev, ch) for rev in (False, True) for ch in "ACGTN"}
    assert {b[12] - 1 for b in blobs} >= set(range(1, 18))                     # name lengths (l_read_name counts the NUL)
    starts, seqs, quals, o = set(), set(), set(), 0
    for b, (l, _, seq_at, qual_at, _) in zip(blobs, lay):
        starts.add(o % 16), seqs.add((o + seq_at) % 16), quals.add((o + qual_at) % 16)
        o += len(b)
    assert starts == seqs == quals == set(range(16))
    no_aux = [qual_at + l == len(b) for b, (l, _, _, qual_at, _) in zip(blobs, lay)]
    assert any(a and b for a, b in zip(no_aux, no_aux[1:])) and not all(no_aux)   # QUAL ends where the next block_size starts
    assert sum(1 for b, (l, _, _, qual_at, fits) in zip(blobs, lay) if l and fits and b[qual_at] == 0xFF) == 2
    cigars = {r.qname: "".join(op for _, op in r.cigar) for r in recs}
    assert cigars["softclip"] == "SMS" and cigars["hardclip"] == "HMH"
    mapq = [b[13] for b in blobs]
    assert any(a >= em.MIN_MQ > b and c >= em.MIN_MQ for a, b, c in zip(mapq, mapq[1:], mapq[2:]))   # a dropped record between kept ones
    # some read is shorter than n5 + n3 and some regions overlap, for every pair of widths but the one-sided ones
    assert all(any(0 < l < n5 + n3 for l, *_ in lay) for n5, n3 in em.WIDTHS if n5 and n3)


@pytest.mark.parametrize("n5,n3", em.WIDTHS)
@pytest.mark.parametrize("mode", em.MODES)
@pytest.mark.parametrize("name", ["crafted", "setA", "setD"])
def test_emulated_kernel(exe, tmp_path, name, mode, n5, n3):
    raw = stream(name)
    (tmp_path / "in.raw").write_bytes(raw)
    pr = subprocess.run([str(exe), str(tmp_path / "in.raw"), str(tmp_path / "out.raw"), mode, str(n5), str(n3)], capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr[-3000:]
    got, want = (tmp_path / "out.raw").read_bytes(), em.mask_stream(raw, mode, n5, n3)
    assert got == want and want != raw


def test_the_restatement_on_records_worked_out_by_hand():
    """TCGTAAT stored on either strand, qualities 30: what the definition gives, written down by hand"""
    def rec(seq, flag, qual="?"):
        return tl.bam_record(tl.Rec(qname="h", flag=flag, rname="c", pos=10, mapq=30, cigar=[(len(seq), "M")], seq=seq, qual=qual * len(seq)), {"c": 0})

    def text(b):
        return em.seq_qual(b)

    fwd, rev = rec("TCGTAAT", 0), rec("TCGTAAT", 16)
    assert text(em.mask_record(fwd, "all", 2, 1)) == ("NNGTAAN", "!!???" + "?!")
    assert text(em.mask_record(rev, "all", 2, 1)) == ("NCGTANN", "!????!!")
    assert text(em.mask_record(fwd, "ds", 3, 3)) == ("NCGTNNT", "!???!!?")          # T in 0..2, A in 4..6
    assert text(em.mask_record(rev, "ds", 3, 3)) == ("NCGTNNT", "!???!!?")          # 3' = stored 0..2: T; 5' = stored 4..6: A
    assert text(em.mask_record(fwd, "ss", 3, 3)) == ("NCGTAAN", "!?????!")          # T at either end
    assert text(em.mask_record(rev, "ss", 3, 3)) == ("TCGTNNT", "????!!?")          # stored A at either end
    assert text(em.mask_record(fwd, "ds", 40)) == ("NCGNNNN", "!??!!!!")            # both regions are the whole read: T or A
    assert text(em.mask_record(fwd, "all", 0, 3))[0] == "TCGTNNN" and text(em.mask_record(rev, "all", 0, 3))[0] == "NNNTAAT"
    odd = em.mask_record(fwd, "all", 0, 1)
    l, _, seq_at, qual_at, _ = em.layout(fwd)
    assert odd[seq_at + 3] == 0xF0 and fwd[seq_at + 3] == 0x80                        # the pad nibble of an odd l_seq stays 0
    assert [i for i in range(len(fwd)) if fwd[i] != odd[i]] == [seq_at + 3, qual_at + 6]
    noq = rec("TCGTAAT", 0, qual="*")[:-7] + b"\xff" * 7
    assert em.seq_qual(em.mask_record(noq, "all", 2, 2)) == ("NNGTANN", "*") and em.mask_record(noq, "all", 2, 2)[-7:] == b"\xff" * 7


@pytest.mark.parametrize("name,mode,n5,n3", [("crafted", "ds", 5, 5), ("crafted", "all", 40, 40), ("setA", "ss", 2, 0), ("setD", "all", 0, 3)])
def test_hostcheck_writes_the_masked_records(bins, tmp_path, name, mode, n5, n3):
    if name == "crafted":
        src = tmp_path / "crafted.bam"
        em.write_raw_bam(src, em.REFS, em.crafted()[1])
    else:
        src = GOLD / f"{name}.bam"
    inflated = tl.bgzf_inflate(src.read_bytes())
    hb = em.header_bytes(inflated)
    assert inflated[hb:] == stream(name)
    plain, masked = tmp_path / "plain.bam", tmp_path / "masked.bam"
    run = lambda out, *more: subprocess.run([str(bins / "hostcheck"), "-a", str(src), "-w", str(out), *more], capture_output=True, text=True, timeout=300)
    p0, p1 = run(plain), run(masked, "-K", f"{mode},{n5},{n3}")
    assert p0.returncode == 0 and p1.returncode == 0, p0.stderr + p1.stderr
    assert p0.stdout == p1.stdout                                        # (the digest is the input's)
    assert gzip.decompress(plain.read_bytes()) == inflated              # without -K: the file it writes today
    got = gzip.decompress(masked.read_bytes())
    assert got == inflated[:hb] + em.mask_stream(inflated[hb:], mode, n5, n3) and got != inflated
    assert masked.read_bytes()[-28:] == tl.BGZF_EOF


def test_hostcheck_with_two_widths_and_with_the_block_path(bins, tmp_path):
    src = GOLD / "setD.bam"
    inflated = tl.bgzf_inflate(src.read_bytes())
    hb = em.header_bytes(inflated)
    for k, more in enumerate((["-K", "all,3"], ["-K", "ds,4,1", "-b"])):
        out = tmp_path / f"o{k}.bam"
        pr = subprocess.run([str(bins / "hostcheck"), "-a", str(src), "-w", str(out), *more], capture_output=True, text=True, timeout=300)
        assert pr.returncode == 0, pr.stderr
        want = em.mask_stream(inflated[hb:], "all", 3, 3) if k == 0 else em.mask_stream(inflated[hb:], "ds", 4, 1)
        assert gzip.decompress(out.read_bytes()) == inflated[:hb] + want


REFUSED = [
    (["-K", "all,2"], "-K (mask the read ends) needs -O"),                       # without -O
    (["-O", "k.bam", "-K", "both,2"], "unknown mode \"both\""),
    (["-O", "k.bam", "-K", "all,0,0"], "both widths are 0"),
    (["-O", "k.bam", "-K", "all,0"], "both widths are 0"),
    (["-O", "k.bam", "-K", "all,70000"], "above 65535"),
    (["-O", "k.bam", "-K", "ds,2,65536"], "above 65535"),
    (["-O", "k.bam", "-K", "all"], "needs the number of bases"),                # a missing count
    (["-O", "k.bam", "-K", "ss,"], "decimal integers"),
    (["-O", "k.bam", "-K", "ss,2,"], "decimal integers"),
    (["-O", "k.bam", "-K", "ss,-2"], "decimal integers"),
    (["-O", "k.bam", "-K", "ss,2,3,4"], "one or two widths"),
    (["-O", "k.bam", "-Z", "-K", "ds,x"], "decimal integers"),
]


@pytest.mark.parametrize("args,message", REFUSED)
def test_cli_refusals(bins, tmp_path, args, message):
    pr = xl.run(bins / "pss-bam", args, tmp_path)
    assert pr.returncode == 1 and pr.stdout == "" and message in pr.stderr and pr.stderr.count("\n") == 1 and pr.stderr.startswith("-K"), pr.stderr
    assert list(tmp_path.iterdir()) == []


def test_usage_names_the_option_and_fragkon_has_none(bins, tmp_path):
    pr = subprocess.run([str(bins / "pss-bam")], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    line = [ln for ln in pr.stderr.splitlines() if ln.startswith("-K ")]
    assert pr.returncode == 1 and len(line) == 1 and "<all|ds|ss>,<n5>[,<n3>]" in line[0] and "with -O" in line[0]
    fk = subprocess.run([str(bins / "fragkon"), "-K", "all,2"], capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert "Unknown option -K." in fk.stderr
    assert list(tmp_path.iterdir()) == []


def test_a_good_K_gets_past_the_option_checks(bins, tmp_path):
    """with -O the option is taken: the command goes on to its inputs, which do not exist here"""
    pr = xl.run(bins / "pss-bam", ["-O", "k.bam", "-K", "ds,3"], tmp_path)
    assert " -O k.bam -z 1 -K ds,3,3\n" in pr.stderr and "-K:" not in pr.stderr and "-K (" not in pr.stderr

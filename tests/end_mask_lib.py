"""pss-bam -K / pssbam_engine_set_end_mask: the definition restated on BAM bytes, and the crafted record set of its tests.

mask_record is the judge of every test of the option: a position-by-position transcription of the definition (include/pssbam_hip.h),
not of the kernel -- it walks all of SEQ and asks of every position whether it lies in the 5' region, in the 3' region, and what
its stored code is.  Nothing in it comes from the engine."""
import struct
from dataclasses import replace

import numpy as np

import mismatch_lib as ml
import pssbam_testlib as tl

MODES = ("all", "ds", "ss")
WIDTHS = [(1, 1), (2, 0), (0, 3), (5, 5), (40, 40)]     # n5 + n3 >= l_seq and overlapping regions both occur on the crafted set
CODE_A, CODE_T, CODE_N = 1, 8, 15


def split_records(raw) -> list:
    b = raw.tobytes() if isinstance(raw, np.ndarray) else bytes(raw)
    out, o = [], 0
    while o < len(b):
        n = 4 + struct.unpack_from("<I", b, o)[0]
        assert o + n <= len(b), "the stream ends inside a record"
        out.append(b[o:o + n])
        o += n
    return out


def layout(rec: bytes):
    """(l_seq, reverse?, SEQ offset, QUAL offset, fields fit?) of a record that starts with its block_size"""
    block_size, = struct.unpack_from("<I", rec, 0)
    l_read_name = rec[12]
    n_cigar_op, flag = struct.unpack_from("<HH", rec, 16)
    l, = struct.unpack_from("<I", rec, 20)
    seq_at = 36 + l_read_name + 4 * n_cigar_op
    qual_at = seq_at + (l + 1) // 2
    return l, bool(flag & 0x10), seq_at, qual_at, qual_at + l <= 4 + block_size


def mask_record(rec: bytes, mode: str, n5: int, n3: int = None) -> bytes:
    n3 = n5 if n3 is None else n3
    assert mode in MODES and len(rec) >= 36 and len(rec) == 4 + struct.unpack_from("<I", rec, 0)[0]
    l, rev, seq_at, qual_at, fits = layout(rec)
    if l == 0 or not fits:
        return bytes(rec)
    out = bytearray(rec)
    has_qual = rec[qual_at] != 0xFF
    k5, k3 = min(n5, l), min(n3, l)
    near = max(k5, k3)
    for i in sorted(set(range(near)) | set(range(l - near, l))):
        in5 = i < k5 if not rev else i >= l - k5
        in3 = i >= l - k3 if not rev else i < k3
        shift = 4 if i % 2 == 0 else 0
        code = (rec[seq_at + i // 2] >> shift) & 15
        if mode == "all":
            masked = in5 or in3
        elif mode == "ds":
            masked = (in5 and code == (CODE_A if rev else CODE_T)) or (in3 and code == (CODE_T if rev else CODE_A))
        else:
            masked = (in5 or in3) and code == (CODE_A if rev else CODE_T)
        if masked:
            out[seq_at + i // 2] |= CODE_N << shift
            if has_qual:
                out[qual_at + i] = 0
    return bytes(out)


def mask_stream(raw, mode: str, n5: int, n3: int = None) -> bytes:
    return b"".join(mask_record(r, mode, n5, n3) for r in split_records(raw))


def seq_qual(rec: bytes):
    """SEQ as text and QUAL as SAM text ('*' when absent) of a well-formed record"""
    l, _, seq_at, qual_at, fits = layout(rec)
    assert fits
    seq = "".join(tl.SEQ_CODES[(rec[seq_at + i // 2] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l))
    q = rec[qual_at:qual_at + l]
    return seq or "*", "*" if (not l or q[0] == 0xFF) else "".join(chr(33 + v) for v in q)


def header_bytes(raw: bytes) -> int:
    """the length of magic + header text + references of an inflated BAM"""
    assert raw[:4] == b"BAM\1"
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    return o


def write_raw_bam(path, refs, raw) -> bytes:
    """a BGZF BAM over the given record bytes (which no tl.Rec need describe); returns the inflated header"""
    head = tl.bam_bytes(refs, [])
    data = head + (raw.tobytes() if isinstance(raw, np.ndarray) else bytes(raw))
    with open(path, "wb") as fh:
        for i in range(0, len(data), 0xFF00):
            fh.write(tl.bgzf_block(data[i:i + 0xFF00], 1))
        fh.write(tl.BGZF_EOF)
    return head


# ---- the crafted set --------------------------------------------------------------------------------------------------------

CONTIG = ml.clean_contig(3000, seed=23)
REFS = [("c", len(CONTIG))]
CONTIGS = [("c", CONTIG)]
LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33]
ENDS = [("A", "T"), ("T", "A"), ("C", "G"), ("G", "C"), ("N", "N"), ("T", "T"), ("A", "A"), ("G", "T"), ("A", "C")]   # (first, last) stored base
MIN_MQ = 20          # the crafted set's run: -q 20 -r 1 -I
REGION_LEN = 1       # (a read is tallied only when it is at least -r long)


def crafted_recs() -> list:
    """tl.Rec list: every length x strand x (first, last) base; name lengths 1..17 in turn; records 4k, 4k+1 without aux fields
    (back to back), the others with an aux field of varying length; every third record MAPQ 10 (dropped under -q 20); then a read
    without SEQ, two without qualities (20 bases: no tool keeps it; one base: kept), a soft-clipped and a hard-clipped one."""
    recs, j = [], 0
    for L in LENGTHS:
        for flag in (0, 16):
            for first, last in ENDS:
                s = 10 + (j * 13) % (len(CONTIG) - 100)
                subs = {L - 1: last, 0: first}
                name = ("r%dxxxxxxxxxxxxxxxxx" % j)[:1 + j % 17]
                r = ml.read_on(CONTIG, s, L, subs, name=name, flag=flag, rname="c", tlen=L, mapq=10 if j % 3 == 2 else 40)
                aux = [] if j % 4 < 2 else [("XZ", "Z", "a" * (j % 7))]
                recs.append(replace(r, qual="".join(chr(33 + 20 + (j + i) % 20) for i in range(L)), tags=aux))
                j += 1
    recs.append(replace(ml.read_on(CONTIG, 200, 20, name="noseq", tlen=20, mapq=40), seq="*", qual="*"))
    recs.append(replace(ml.read_on(CONTIG, 300, 20, {0: "T", 19: "A"}, name="noqual", tlen=20, mapq=40), qual="*"))
    # (SAM text cannot tell absent qualities from Phred 9 on a one-base read, so the tools keep that one read without qualities)
    recs.append(replace(ml.read_on(CONTIG, 350, 1, {0: "T"}, name="noqual1", tlen=1, mapq=40), qual="*"))
    soft = ml.read_on(CONTIG, 400, 20, name="softclip", tlen=20, mapq=40)
    recs.append(replace(soft, cigar=[(3, "S"), (20, "M"), (2, "S")], seq="TTT" + soft.seq + "AA", qual="I" * 25))
    hard = ml.read_on(CONTIG, 500, 20, {0: "T", 19: "A"}, name="hardclip", flag=16, tlen=20, mapq=40)
    recs.append(replace(hard, cigar=[(4, "H"), (20, "M"), (3, "H")]))
    return recs


_CRAFTED = {}


def crafted():
    """(recs, raw, indices of the malformed records in the stream): the records of crafted_recs() as BAM bytes, and in the middle
    two records more whose l_seq claims more than the record holds: by two bytes (SEQ and QUAL would end in the aux field's last
    bytes and behind it) and by far.  The engine decodes such a record as unmapped (csrc/record_decode.h decode_hdr), so no run
    keeps it: the bounds rule is exercised where the stream is masked without a selection in front -- the emulated kernel and
    hostcheck -- and not on the device."""
    if not _CRAFTED:
        recs = crafted_recs()
        blobs = [tl.bam_record(r, {"c": 0}) for r in recs]
        at = len(blobs) // 2
        for k, l_seq in enumerate((7, 1001)):     # recs[3]: one base, an aux field of 7 bytes: l_seq 6 would fit, 7 does not
            bad = bytearray(tl.bam_record(replace(recs[3], qname="malformed", mapq=40), {"c": 0}))
            assert layout(bytes(bad))[0] == 1 and len(bad) == layout(bytes(bad))[3] + 1 + 7
            struct.pack_into("<I", bad, 20, l_seq)
            assert not layout(bytes(bad))[4]
            blobs.insert(at + k, bytes(bad))
        _CRAFTED["v"] = (recs, np.frombuffer(b"".join(blobs), dtype=np.uint8), [at, at + 1])
    return _CRAFTED["v"]

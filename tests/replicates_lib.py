"""pss-bam -J in Python: the read-name hash that picks a record's replicate, the reduction of a record list to one
replicate, and the delete-one-group jackknife over the replicates' tables.  Restated from the definitions in
include/pssbam_hip.h and pss-bam_amd/host/replicates.h, not from their code."""
import struct

import numpy as np

import pssbam_testlib as tl

M32 = 0xFFFFFFFF
VECTORS = {b"": 0xab3e7c0b, b"a": 0x2a681819, b"read/1": 0x9d5b3ad0, b"r0000000": 0x4620f828}
OFF_DIAG = (1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14)   # cells of AC AG AT CA CG CT GA GC GT TA TC TG; cell & 3 = reference base


def name_hash(name: bytes) -> int:
    n = len(name)
    h = 2166136261
    for i in range(0, n, 4):
        w = int.from_bytes(name[i:i + 4], "little")       # a short last word is zero-filled
        h = ((h ^ w) * 16777619) & M32
    h ^= n
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def replicate(name, k: int) -> int:
    if isinstance(name, str):
        name = name.encode()
    return (name_hash(name) * k) >> 32


def reduce(recs, k: int, j: int) -> list:
    """the records of replicate j among k, in input order"""
    return [r for r in recs if replicate(r.qname, k) == j]


def reduce_sam_text(text: str, k: int, j: int) -> str:
    """a SAM text with its header lines and the alignment lines of replicate j"""
    return "".join(ln for ln in text.splitlines(keepends=True) if ln.startswith("@") or replicate(ln.split("\t", 1)[0], k) == j)


def sub_rates(counts: np.ndarray) -> np.ndarray:
    """(N, 12) rates of an (N + 2, 16) table: count / column total of the reference base; a position with an empty A, C, G
    or T column keeps twelve zeros"""
    counts = np.asarray(counts, dtype=np.uint64)
    n = counts.shape[0] - 2
    out = np.zeros((n, 12), dtype=np.float64)
    for pos in range(n):
        row = counts[pos + 2]
        col = [int(row[ref]) + int(row[4 + ref]) + int(row[8 + ref]) + int(row[12 + ref]) for ref in range(4)]
        if 0 in col:
            continue
        for c, cell in enumerate(OFF_DIAG):
            out[pos, c] = int(row[cell]) / col[cell & 3]
    return out


def jackknife_se(total: np.ndarray, planes: np.ndarray) -> np.ndarray:
    """(N, 12) standard errors from the total (N + 2, 16) and the K replicate tables (K, N + 2, 16)"""
    total, planes = np.asarray(total, dtype=np.uint64), np.asarray(planes, dtype=np.uint64)
    k = planes.shape[0]
    theta = np.stack([sub_rates(total - planes[j]) for j in range(k)])
    mean = theta.sum(axis=0) / k
    return np.sqrt((k - 1) / k * ((theta - mean) ** 2).sum(axis=0))


def parse_rates_text(text: str):
    """the '###' lines and the (labels, (n, 12) values as printed) of the two blocks of a rates-layout file"""
    lines = text.split("\n")
    assert lines[-1] == ""
    head = [ln for ln in lines if ln.startswith("###")]
    blocks, cur = [], None
    for ln in lines[:-1]:
        if ln.startswith("###") or ln == "":
            if cur:
                blocks.append(cur)
            cur = None
            continue
        f = ln.split("\t")
        assert len(f) == 14 and f[13] == "", ln          # every row ends in a TAB
        cur = cur or []
        cur.append((int(f[0]), f[1:13]))
    if cur:
        blocks.append(cur)
    assert len(blocks) == 2
    return head, [([lab for lab, _ in b], [v for _, v in b]) for b in blocks]


def raw_record(name: bytes, ref_id: int, pos0: int, seq: str, mapq: int = 30, flag: int = 0) -> bytes:
    """a <len>M BAM record whose read name is any byte string (its closing NUL is added here)"""
    l_seq = len(seq)
    codes = [tl.SEQ_CODES.index(ch) for ch in seq] + ([0] if l_seq & 1 else [])
    seq_b = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    core = struct.pack("<iiBBHHHIiii", ref_id, pos0, len(name) + 1, mapq, 4681, 1, flag, l_seq, -1, -1, 0)
    body = core + name + b"\0" + struct.pack("<I", l_seq << 4) + seq_b + bytes([40]) * l_seq
    return struct.pack("<I", len(body)) + body

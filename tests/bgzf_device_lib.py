"""Fixtures for the public device-buffer BGZF entry point, pssbam_bgzf_inflate_device (include/pssbam_hip.h), and for
the edge arithmetic of the three CRC-32 kernels behind launch_crc (csrc/bgzf_api.h, csrc/inflate_kernels.h):

* block()              one BGZF block whose trailer may describe OTHER bytes than its payload inflates to -- the decoder
                       then reports status 0 and only the CRC check can refuse the block;
* EDGE_SIZES           the ISIZE values at which bgzf_crc_lines_kernel (head / 16-byte pieces dealt to 64 lanes, 8 x 64 per
                       loop trip / tail) and bgzf_crc_kernel (1 KiB chunks counted from the block's end) change branch;
* layout()             a caller's block table: every block at a chosen out_off & 15, guard bytes between the blocks, the
                       blocks placed in reversed order;
* changed_positions()  the bytes of a block whose damage each arm of the kernels has to notice;
* run_device()         torch tensors for the three buffers (canary-filled output, 64 filled bytes behind comp_bytes) and the
                       call itself;
* crc_matrix()         every (size, alignment, changed position) in one launch.  `python tests/bgzf_device_lib.py
                       --crc-matrix` runs it in a process of its own: PSSBAM_CRC_FORM is read once per process, so the
                       chunk-per-lane kernel is reached from a fresh child (crc_matrix_child).

Reference for everything: zlib (zlib.decompress(..., -15), zlib.crc32); all comparisons are exact.
tests/test_bgzf_device_host.py proves this file on the CPU.  Nothing here needs a GPU, or torch, at import."""
import json
import os
import struct
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
BGZF_HEAD = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"
BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("in_len", "<u4"), ("isize", "<u4"), ("out_off", "<u8"), ("crc", "<u4"), ("status", "<u4")])
assert BLOCK_DTYPE.itemsize == 32          # sizeof(pssbam_bgzf_block)
CANARY = 0xA5
COMP_SLACK = 64                            # bytes the compressed tensor is longer than comp_bytes
INF_OK, INF_BAD_BLOCK, INF_TRUNCATED, INF_BAD_CRC = 0, 1, 7, 8
PSSBAM_OK, PSSBAM_EINVAL = 0, -1
ALPHABET = np.frombuffer(b"ACGT", dtype=np.uint8)

EDGE_SIZES = ([0, 1, 2, 15, 16, 17, 31, 32, 33]
              + list(range(1007, 1042))           # 16 * 63, 16 * 64, 16 * 65 pieces with every tail; the first 1 KiB chunk boundary +- 1
              + [2047, 2048, 2049]
              + [8175, 8176, 8191, 8192, 8193, 8207, 8208, 8209]   # 8 * 64 pieces (one loop trip of the lines kernel) +- 1 piece, +- 1 byte
              + [16383, 16384, 16385]
              + [64511, 64512, 64513]             # 64513: lane 0 of the chunk kernel owns exactly one byte
              + [65519, 65520, 65535, 65536])


def payload_bytes(rng, n: int) -> bytes:
    """n bytes of a 4-letter alphabet: 64 KiB of them deflate to well under the BGZF block limit at level 1"""
    return ALPHABET[rng.integers(0, 4, n)].tobytes()


def change_byte(data: bytes, at: int) -> bytes:
    """`data` with the byte at `at` replaced by another letter of the alphabet (an 8-bit burst: CRC-32 must notice)"""
    b = bytearray(data)
    b[at] = b"CGTA"[b"ACGT".index(b[at])] if b[at] in b"ACGT" else b[at] ^ 0x5A
    return bytes(b)


def block(data: bytes, level: int = 1, trailer_of: bytes | None = None, crc: int | None = None) -> bytes:
    """One BGZF block whose payload deflates `data`; CRC-32 and ISIZE in its trailer are those of `trailer_of` (default:
    of `data`).  crc: the CRC field as given (the empty block with a non-zero CRC)."""
    t = data if trailer_of is None else trailer_of
    assert len(t) == len(data), "the trailer's ISIZE must be what the payload inflates to: only the CRC may disagree"
    small = len(data) <= 256        # (a 512-byte window and a 256-entry hash: tables of ~10^5 tiny blocks are built in a second)
    co = zlib.compressobj(level, zlib.DEFLATED, -9 if small else -15, 1 if small else 8)
    payload = co.compress(data) + co.flush()
    bsize = len(payload) + 25       # the BC field: block length - 1
    assert bsize < 65536
    return (BGZF_HEAD + struct.pack("<H", bsize) + payload
            + struct.pack("<II", (zlib.crc32(t) & 0xFFFFFFFF) if crc is None else crc, len(t)))


def parse_block(b: bytes):
    """(payload offset in the block, payload length, crc field, isize field) of one block built by block()"""
    xlen = struct.unpack_from("<H", b, 10)[0]
    assert b[:4] == BGZF_HEAD[:4] and struct.unpack_from("<H", b, 16)[0] + 1 == len(b)
    crc, isize = struct.unpack_from("<II", b, len(b) - 8)
    return 12 + xlen, len(b) - 12 - xlen - 8, crc, isize


def changed_positions(T: int, align: int = 0) -> list[int]:
    """positions of a T-byte block at out_off & 15 == align whose damage the CRC kernels' arms must each notice: around the
    head (the bytes in front of the first 16-byte aligned piece), the first pieces, piece 63 / 64 (the second round of the 64
    lanes), piece 511 / 512 (the second loop trip), the chunk kernel's last 1 KiB boundary, the last piece and the tail"""
    if T <= 33:
        return list(range(T))
    head = min((16 - align) & 15, T)
    cand = [0, head - 1, head, head + 15, head + 16, head + 16 * 63 + 15, head + 16 * 64, head + 16 * 512 - 1, head + 16 * 512,
            T - 1025, T - 1024, T - 1023, T - 17, T - 16, T - 1]
    return sorted({p for p in cand if 0 <= p < T})


def layout(sizes, aligns, gap):
    """A caller's block table (BLOCK_DTYPE) for blocks of `sizes` bytes: block i sits at an out_off with out_off & 15 ==
    aligns[i], the smallest one that leaves at least gap (an int, or one per block) guard bytes behind whatever lies in front
    of it, and the blocks are placed in REVERSED order -- the last block of the table lowest.  Returns (table, out_bytes);
    out_bytes leaves the last gap behind the highest block.  in_off / in_len / crc are the caller's to fill."""
    n = len(sizes)
    gaps = [int(gap)] * n if np.isscalar(gap) else [int(g) for g in gap]
    assert len(aligns) == n and len(gaps) == n
    tab = np.zeros(n, dtype=BLOCK_DTYPE)
    off = np.zeros(n, dtype=np.uint64)
    cur = 0
    for i in range(n - 1, -1, -1):
        cur += gaps[i]
        cur += (int(aligns[i]) - cur) & 15
        off[i] = cur
        cur += int(sizes[i])
    tab["out_off"] = off
    tab["isize"] = np.asarray(sizes, dtype=np.uint32)
    return tab, cur + (gaps[0] if n else 0)


def table_of(blocks, aligns, gap, cut_last_trailer: bool = False):
    """(comp bytes, comp_bytes, table, out_bytes) for whole BGZF blocks laid end to end in the compressed buffer and laid
    out by layout() in the output.  cut_last_trailer: comp_bytes ends with the last block's payload."""
    parsed = [parse_block(b) for b in blocks]
    tab, out_bytes = layout([p[3] for p in parsed], aligns, gap)
    starts = np.concatenate([[0], np.cumsum([len(b) for b in blocks])]).astype(np.uint64)
    tab["in_off"] = starts[:-1] + np.array([p[0] for p in parsed], dtype=np.uint64)
    tab["in_len"] = np.array([p[1] for p in parsed], dtype=np.uint32)
    tab["crc"] = np.array([p[2] for p in parsed], dtype=np.uint32)
    comp = b"".join(blocks)
    comp_bytes = len(comp) - (8 if cut_last_trailer and blocks else 0)
    return np.frombuffer(comp, dtype=np.uint8), comp_bytes, tab, out_bytes


def expected_output(tab, datas, out_bytes: int, canary: int = CANARY) -> np.ndarray:
    """the whole output buffer as it must look: canary everywhere but in the ranges of the blocks whose datas[i] is not None"""
    want = np.full(out_bytes, canary, dtype=np.uint8)
    for o, d in zip(tab["out_off"].tolist(), datas):
        if d:
            want[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    return want


def first_difference(got: np.ndarray, want: np.ndarray, tab) -> str | None:
    """None, or where the first wrong byte of the output buffer lies relative to the blocks of the table"""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return f"output has {got.size} bytes, expected {want.size}"
    at = int(np.flatnonzero(got != want)[0])
    off, size = tab["out_off"].astype(np.int64), tab["isize"].astype(np.int64)
    inside = np.flatnonzero((off <= at) & (at < off + size))
    if inside.size:
        i = int(inside[0])
        return f"byte {at}: {at - int(off[i])} of block {i} ({int(size[i])} bytes at out_off {int(off[i])}): got {int(got[at])}, want {int(want[at])}"
    below = np.flatnonzero(off + size <= at)
    near = int(below[np.argmax((off + size)[below])]) if below.size else None
    return (f"guard byte {at} changed to {int(got[at])}" + (f", {at - int((off + size)[near])} bytes behind the end of block {near}" if near is not None else
                                                              ", in front of every block"))


# ---------------------------------------------------------------------------------------------------------------------
# the device side (torch only inside)
# ---------------------------------------------------------------------------------------------------------------------
def load_pkg():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    assert pkg.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return pkg


def entry_point(pkg):
    import ctypes as C
    L = pkg.hip_lib()
    L.pssbam_bgzf_inflate_device.restype = C.c_int
    L.pssbam_bgzf_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    return L.pssbam_bgzf_inflate_device


def upload(comp: np.ndarray, comp_bytes: int, tab: np.ndarray, out_bytes: int, tail_fill: int = 0, canary: int = CANARY):
    """(d_comp, d_blocks, d_out): the compressed tensor is COMP_SLACK bytes longer than comp_bytes, filled with tail_fill
    there (whatever `comp` holds behind comp_bytes does not go up); the output tensor holds the canary"""
    import torch
    dev = torch.device("cuda", 0)
    d_comp = torch.full((comp_bytes + COMP_SLACK,), tail_fill, dtype=torch.uint8, device=dev)
    if comp_bytes:
        d_comp[:comp_bytes] = torch.from_numpy(np.array(comp[:comp_bytes], dtype=np.uint8)).to(dev)
    d_blocks = torch.from_numpy(np.ascontiguousarray(tab).view(np.uint8).copy()).to(dev) if len(tab) else torch.zeros(32, dtype=torch.uint8, device=dev)
    d_out = torch.full((max(out_bytes, 1),), canary, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    return d_comp, d_blocks, d_out


def call(pkg, d_comp, comp_bytes: int, d_blocks, n_blocks: int, d_out, check_crc: int, own_stream: bool = False, comp_shift: int = 0,
         null: str | None = None) -> int:
    """pssbam_bgzf_inflate_device on stream 0 or on a torch stream of its own; returns after the work has run.
    comp_shift: added to d_comp's address; null: which of "comp" / "blocks" / "out" goes in as a null pointer."""
    import torch
    fn = entry_point(pkg)
    ptr = {"comp": d_comp.data_ptr() + comp_shift, "blocks": d_blocks.data_ptr(), "out": d_out.data_ptr()}
    if null:
        ptr[null] = None
    if own_stream:
        s = torch.cuda.Stream()
        rc = fn(s.cuda_stream, ptr["comp"], comp_bytes, ptr["blocks"], n_blocks, ptr["out"], check_crc)
        s.synchronize()
    else:
        rc = fn(0, ptr["comp"], comp_bytes, ptr["blocks"], n_blocks, ptr["out"], check_crc)
    torch.cuda.synchronize()
    return int(rc)


def run_device(pkg, comp, comp_bytes, tab, out_bytes, check_crc, tail_fill=0, canary=CANARY, own_stream=False):
    """upload + call + download: (return code, the statuses, the whole output buffer)"""
    d_comp, d_blocks, d_out = upload(comp, comp_bytes, tab, out_bytes, tail_fill, canary)
    rc = call(pkg, d_comp, comp_bytes, d_blocks, len(tab), d_out, check_crc, own_stream)
    status = d_blocks.cpu().numpy()[:32 * len(tab)].view(BLOCK_DTYPE)["status"].copy()
    return rc, status, d_out.cpu().numpy()[:out_bytes]


# ---------------------------------------------------------------------------------------------------------------------
# the CRC matrix
# ---------------------------------------------------------------------------------------------------------------------
def matrix_alignments(T: int):
    """all sixteen up to 2049 bytes, four above: 47 MB of inflated data in all, so nothing else had to be dropped"""
    return list(range(16)) if T <= 2049 else [0, 1, 8, 15]


def crc_matrix_cases(seed: int = 2024):
    """[(T, align, changed position or None, block bytes, what the payload inflates to, wanted status)]: per size and
    alignment one intact block and one block per changed position whose trailer is the intact block's; T = 0 with CRC
    field 0 and with a non-zero one"""
    rng = np.random.default_rng(seed)
    cases = []
    for T in EDGE_SIZES:
        for a in matrix_alignments(T):
            data = payload_bytes(rng, T)
            cases.append((T, a, None, block(data, 1), data, INF_OK))
            for p in changed_positions(T, a):
                other = change_byte(data, p)
                cases.append((T, a, p, block(other, 1, trailer_of=data), other, INF_BAD_CRC))
            if T == 0:
                cases.append((T, a, "crc", block(b"", 1, crc=0x1D0F5EED), b"", INF_BAD_CRC))
    return cases


def crc_matrix(pkg, cases=None) -> dict:
    """the matrix through pssbam_bgzf_inflate_device with check_crc = 1, one launch: {"checked": blocks, "failures": [...]}"""
    cases = cases or crc_matrix_cases()
    comp, comp_bytes, tab, out_bytes = table_of([c[3] for c in cases], [c[1] for c in cases], 3)
    rc, status, out = run_device(pkg, comp, comp_bytes, tab, out_bytes, 1)
    failures = []
    if rc != PSSBAM_OK:
        failures.append(f"pssbam_bgzf_inflate_device returned {rc}")
    want_status = np.array([c[5] for c in cases], dtype=np.uint32)
    for i in np.flatnonzero(status != want_status)[:40].tolist():
        T, a, p = cases[i][:3]
        failures.append(f"T={T} align={a} changed={p}: status {int(status[i])}, expected {int(want_status[i])}")
    diff = first_difference(out, expected_output(tab, [c[4] for c in cases], out_bytes), tab)
    if diff:
        failures.append("output differs from zlib's: " + diff)
    return {"checked": len(cases), "failures": failures}


def crc_matrix_child(env_extra: dict, timeout: float = 600.0):
    """the matrix in a fresh process started with env_extra set: (exit code, the JSON line or None, stderr)"""
    env = {k: v for k, v in os.environ.items() if k not in ("PSSBAM_CRC_FORM", "PSSBAM_CRC_WAVES")}
    env.update(env_extra)
    argv = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [str(Path(__file__).resolve()), "--crc-matrix"]
    pr = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, env=env)
    lines = [ln for ln in pr.stdout.splitlines() if ln.startswith("{")]
    return pr.returncode, json.loads(lines[-1]) if lines else None, pr.stderr


if __name__ == "__main__":
    if sys.argv[1:] != ["--crc-matrix"]:
        sys.exit(f"usage: {sys.argv[0]} --crc-matrix")
    res = crc_matrix(load_pkg())
    print(json.dumps(res))
    sys.exit(0 if not res["failures"] else 1)

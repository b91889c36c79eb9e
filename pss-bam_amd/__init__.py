"""ctypes face of the MI355X tally engine (libpssbam_hip.so, include/pssbam_hip.h).

This module is thin plumbing for tests/, bench.py and __graft_entry__: it loads the
C-ABI shared library and marshals arguments.  There is no computation here and no CPU
fallback: if the library (or a gfx950 device) is missing, construction raises.

The directory name contains a hyphen, so import it through `load_pkg()` in
__graft_entry__.py (importlib by path) under the module name `pss_bam_amd`.
"""
from __future__ import annotations

import ctypes as C
import subprocess
from dataclasses import dataclass
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
ROOT = PKG_DIR.parent
LIB_HIP = PKG_DIR / "libpssbam_hip.so"
LIB_HOST = PKG_DIR / "libpssbam_host.so"
LIB_SYNTH = PKG_DIR / "libpssbam_synth.so"

TALLY_PSS, TALLY_KMER = 1, 2
KERNEL_AUTO, KERNEL_SIMPLE, KERNEL_TILED = 0, 1, 2
ST_NAMES = ["records", "rg_dropped", "parse_skip", "no_contig", "pss_ok", "pss_filtered", "kmer_ok",
            "kmer_filtered", "kmer_fail", "slow_path"]
ST_N = 16

# every symbol include/pssbam_hip.h declares (checked by tests/test_cabi.py)
HIP_SYMBOLS = [
    "pssbam_last_error", "pssbam_device_count", "pssbam_warmup", "pssbam_engine_create", "pssbam_engine_destroy",
    "pssbam_engine_set_stream", "pssbam_engine_set_genome", "pssbam_engine_set_genome_arrays",
    "pssbam_engine_set_references", "pssbam_engine_submit", "pssbam_engine_submit_async", "pssbam_engine_wait_copied",
    "pssbam_engine_copy_done", "pssbam_engine_phase_times", "pssbam_engine_submit_device", "pssbam_engine_sync",
    "pssbam_engine_finish", "pssbam_engine_reset", "pssbam_engine_counters_device", "pssbam_engine_bind_counters",
    "pssbam_reduce_counters", "pssbam_engine_genome_kmer_count", "pssbam_host_register", "pssbam_host_unregister", "pssbam_engine_timer_begin",
    "pssbam_engine_timer_end", "pssbam_engine_kernel_time", "pssbam_index_records", "pssbam_bgzf_scan",
    "pssbam_bgzf_inflate_device", "pssbam_bgzf_inflate_host", "pssbam_engine_submit_bgzf", "pssbam_engine_wait_bgzf_copied",
    "pssbam_engine_feed_status", "pssbam_engine_feed_break", "pssbam_engine_feed_handoff", "pssbam_feed_reserve", "pssbam_engine_hint_records",
    "pssbam_engine_set_genome_async", "pssbam_engine_genome_wait", "pssbam_engine_feed_open", "pssbam_feed_release",
    "pssbam_engine_set_read_groups", "pssbam_engine_finish_groups", "pssbam_engine_set_length_bins",
    "pssbam_engine_set_contig_sets", "pssbam_engine_finish_kmer_groups", "pssbam_engine_set_min_base_quality",
    "pssbam_engine_set_regions", "pssbam_engine_set_length_histogram", "pssbam_engine_finish_length_histogram",
    "pssbam_engine_set_site_context", "pssbam_engine_finish_site_context",
    "pssbam_engine_set_end_condition", "pssbam_engine_finish_end_condition", "pssbam_engine_set_gapped_reads",
    "pssbam_engine_set_per_contig", "pssbam_engine_finish_contigs",
    "pssbam_engine_set_mismatches", "pssbam_engine_finish_mismatches", "pssbam_engine_set_replicates",
    "pssbam_engine_set_interior", "pssbam_engine_finish_interior",
    "pssbam_engine_set_composition", "pssbam_engine_finish_composition",
    "pssbam_engine_set_read_score", "pssbam_engine_finish_read_score",
    "pssbam_engine_set_record_sink", "pssbam_engine_set_block_sink", "pssbam_engine_set_end_mask",
    "pssbam_engine_set_duplicates", "pssbam_engine_finish_duplicates",
    "pssbam_engine_set_coverage", "pssbam_engine_finish_coverage", "pssbam_engine_finish_coverage_runs",
    "pssbam_engine_finish_coverage_windows",
    "pssbam_engine_set_sites", "pssbam_engine_finish_sites",
    "pssbam_bgzf_deflate_work_bytes", "pssbam_bgzf_deflate_device", "pssbam_bgzf_deflate_host",
]
MAX_READ_GROUPS = 4096
MAX_LENGTH_BINS = 64
MAX_CONTIG_SETS = 4096
MAX_REPLICATES = 64
MAX_BASE_QUALITY = 93
MAX_HIST_LENGTH = 65535
MAX_MISMATCHES = 255
MAX_INTERIOR_MARGIN = 65535
MAX_COMPOSITION = 30
MAX_SCORE_DIST = 64
MAX_SCORE_QUAL = 64
MAX_SCORE_WEIGHT = 2047
MAX_SCORE_HALF = 128
MAX_REGIONS = 1 << 26
SITE_NONE, SITE_CPG = 0, 1
SITE_MODES = {None: SITE_NONE, "none": SITE_NONE, "cpg": SITE_CPG}
MAX_END_DEPTH = 8
END_MASK_OFF, END_MASK_ALL, END_MASK_DS, END_MASK_SS = 0, 1, 2, 3
END_MASK_MODES = {None: END_MASK_OFF, "off": END_MASK_OFF, "all": END_MASK_ALL, "ds": END_MASK_DS, "ss": END_MASK_SS}
MAX_END_MASK = 65535
RESCALE_OFF, RESCALE_DS, RESCALE_SS = 0, 1, 2
RESCALE_MODES = {None: RESCALE_OFF, "off": RESCALE_OFF, "ds": RESCALE_DS, "ss": RESCALE_SS}
MAX_RESCALE_ROWS, RESCALE_QUALS = 64, 94
MAX_DUP_HIST = 65535
COV_HIST_MAX = 255
MAX_SITE_TRIM = 65535
END_PRESETS = {"ss": (13, 13), "ds": (13, 2)}   # (cell5, cell3): C->T at both ends / C->T at the 5' end, G->A at the 3' end
GAPPED_TILED_OPS = 16   # pss-bam -I: CIGAR ops a lane of the tiled kernel walks (csrc/record_decode.h); more take the one-lane path
EBUSY = -7


def build(verbose: bool = False) -> None:
    """make -C pss-bam_amd: compiles every HIP extension for gfx950 plus the host C side."""
    subprocess.run(["make", "-C", str(PKG_DIR), "all"], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)


class PssbamError(RuntimeError):
    pass


class _PssOpts(C.Structure):
    _fields_ = [("region_len", C.c_int32), ("min_read_len", C.c_uint64), ("max_read_len", C.c_uint64),
                ("min_mq", C.c_int32), ("up_ctx", C.c_char_p), ("down_ctx", C.c_char_p),
                ("merged_only", C.c_int32)]


class _KmerOpts(C.Structure):
    _fields_ = [("klen", C.c_int32), ("min_mq", C.c_int32), ("min_read_len", C.c_uint64),
                ("max_read_len", C.c_uint64), ("merged_only", C.c_int32)]


class _Config(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("tally_mask", C.c_uint32), ("pss", _PssOpts), ("kmer", _KmerOpts),
                ("read_group", C.c_char_p), ("device", C.c_int32), ("kernel", C.c_int32)]


_RECORD_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64)   # pssbam_record_sink

_BLOCK_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64)   # pssbam_block_sink

_hip = None


def hip_lib() -> C.CDLL:
    """Loads libpssbam_hip.so; raises (loudly) when it has not been built."""
    global _hip
    if _hip is not None:
        return _hip
    if not LIB_HIP.exists():
        raise PssbamError(f"{LIB_HIP} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    L = C.CDLL(str(LIB_HIP))
    L.pssbam_last_error.restype = C.c_char_p
    L.pssbam_engine_create.argtypes = [C.POINTER(_Config), C.POINTER(C.c_void_p)]
    L.pssbam_engine_destroy.argtypes = [C.c_void_p]
    L.pssbam_engine_destroy.restype = None
    L.pssbam_engine_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_genome.argtypes = [C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_genome_arrays.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_int]
    L.pssbam_engine_set_references.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p)]
    L.pssbam_engine_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
    L.pssbam_engine_submit_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    L.pssbam_engine_wait_copied.argtypes = [C.c_void_p, C.c_uint64]
    L.pssbam_engine_copy_done.argtypes = [C.c_void_p, C.c_uint64]
    L.pssbam_engine_phase_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
                                            C.POINTER(C.c_uint64)]
    L.pssbam_engine_submit_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]
    L.pssbam_engine_sync.argtypes = [C.c_void_p]
    L.pssbam_engine_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_reset.argtypes = [C.c_void_p]
    L.pssbam_engine_set_read_groups.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p)]
    L.pssbam_engine_finish_groups.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.pssbam_engine_finish_kmer_groups.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_length_bins.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_uint32)]
    L.pssbam_engine_set_contig_sets.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]
    L.pssbam_engine_set_min_base_quality.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_set_length_histogram.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_finish_length_histogram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_site_context.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_finish_site_context.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_end_condition.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    L.pssbam_engine_finish_end_condition.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_gapped_reads.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_set_per_contig.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_set_replicates.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_set_mismatches.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    L.pssbam_engine_finish_mismatches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_interior.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_finish_interior.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_composition.argtypes = [C.c_void_p, C.c_int32]
    L.pssbam_engine_finish_composition.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_read_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.pssbam_engine_finish_read_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_finish_contigs.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_set_regions.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_engine_counters_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.pssbam_engine_bind_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.pssbam_engine_genome_kmer_count.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.pssbam_engine_timer_begin.argtypes = [C.c_void_p]
    L.pssbam_engine_timer_end.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.pssbam_engine_kernel_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]
    if hasattr(L, "pssbam_engine_set_record_sink"):   # (tools/select_bench.py also loads the library of the commit before the sink)
        L.pssbam_engine_set_record_sink.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "pssbam_engine_set_block_sink"):   # (tools/deflate_bench.py also loads the library of the commit before it)
        L.pssbam_engine_set_block_sink.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.pssbam_bgzf_deflate_work_bytes.restype = C.c_uint64
        L.pssbam_bgzf_deflate_work_bytes.argtypes = [C.c_uint64]
        L.pssbam_bgzf_deflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]
        L.pssbam_bgzf_deflate_host.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_int]
    if hasattr(L, "pssbam_engine_set_end_mask"):   # (tools/end_mask_bench.py also loads the library of the commit before it)
        L.pssbam_engine_set_end_mask.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_uint32]
    L.pssbam_index_records.restype = C.c_int64
    if hasattr(L, "pssbam_engine_set_duplicates"):   # (tools/dedup_bench.py also loads the library of the commit before it)
        L.pssbam_engine_set_duplicates.argtypes = [C.c_void_p, C.c_int32, C.c_uint32]
        L.pssbam_engine_finish_duplicates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    if hasattr(L, "pssbam_engine_set_coverage"):   # (tools/coverage_bench.py also loads the library of the commit before it)
        L.pssbam_engine_set_coverage.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
        L.pssbam_engine_finish_coverage.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.pssbam_engine_finish_coverage_runs.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "pssbam_engine_finish_coverage_windows"):   # (tools/windows_bench.py also loads the library of the commit before it)
        L.pssbam_engine_finish_coverage_windows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 8
    if hasattr(L, "pssbam_engine_set_sites"):   # (tools/allele_bench.py also loads the library of the commit before it)
        L.pssbam_engine_set_sites.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.c_int64, C.c_void_p, C.c_void_p, C.c_uint32]
        L.pssbam_engine_finish_sites.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pssbam_index_records.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    _hip = L
    return L


def _chk(rc: int) -> None:
    if rc != 0:
        raise PssbamError(f"pssbam error {rc}: {hip_lib().pssbam_last_error().decode()}")


def bgzf_inflate(bgzf: np.ndarray, check_crc: bool = True, repeats: int = 1, want_output: bool = True) -> dict:
    """Inflates whole BGZF blocks on the GPU (pssbam_bgzf_inflate_host): {"data", "n_blocks", "bad_block",
    "bad_status", "kernel_ms"}; bad_block is None when every block passed."""
    L = hip_lib()
    L.pssbam_bgzf_inflate_host.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_double), C.c_int, C.c_int]
    L.pssbam_bgzf_scan.restype = C.c_int64
    L.pssbam_bgzf_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    bgzf = np.ascontiguousarray(bgzf, dtype=np.uint8)
    consumed, total = C.c_uint64(), C.c_uint64()
    n = L.pssbam_bgzf_scan(bgzf.ctypes.data, bgzf.size, None, 0, C.byref(consumed), C.byref(total))
    if n < 0:
        _chk(int(n))
    out = np.empty(int(total.value) if want_output else 0, dtype=np.uint8)
    out_len, nb, bad_b, bad_s, ms = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_double()
    _chk(L.pssbam_bgzf_inflate_host(-1, bgzf.ctypes.data, bgzf.size, out.ctypes.data if want_output else None, out.size,
                                    C.byref(out_len), C.byref(nb), C.byref(bad_b), C.byref(bad_s), C.byref(ms),
                                    int(check_crc), repeats))
    return {"data": out, "inflated_bytes": int(out_len.value), "n_blocks": int(nb.value),
            "bad_block": None if bad_b.value == 0xFFFFFFFF else int(bad_b.value), "bad_status": int(bad_s.value),
            "kernel_ms": float(ms.value)}


BGZF_PAYLOAD = 0xFF00   # bytes of the stream per block of the device deflate


def bgzf_deflate(raw: np.ndarray, repeats: int = 1) -> dict:
    """Deflates bytes into whole BGZF blocks on the GPU (pssbam_bgzf_deflate_host), cut every 0xFF00 bytes: {"data" (the
    blocks back to back, no EOF block), "n_blocks", "kernel_ms"}."""
    L = hip_lib()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    n_blocks = (raw.size + BGZF_PAYLOAD - 1) // BGZF_PAYLOAD
    out = np.empty(raw.size + 31 * n_blocks, dtype=np.uint8)   # (no block is larger than its stored form)
    out_len, nb, ms = C.c_uint64(), C.c_uint32(), C.c_double()
    _chk(L.pssbam_bgzf_deflate_host(-1, raw.ctypes.data if raw.size else None, raw.size, out.ctypes.data if out.size else None, out.size,
                                    C.byref(out_len), C.byref(nb), C.byref(ms), repeats))
    return {"data": out[:int(out_len.value)].copy(), "n_blocks": int(nb.value), "kernel_ms": float(ms.value)}


def bgzf_deflate_device(hip_stream: int, d_raw: int, raw_bytes: int, d_bgzf: int, bgzf_cap: int, d_totals: int, d_work: int, work_bytes: int):
    """pssbam_bgzf_deflate_device on device pointers (e.g. torch tensors' data_ptr()); bgzf_deflate_work_bytes() sizes d_work"""
    _chk(hip_lib().pssbam_bgzf_deflate_device(C.c_void_p(hip_stream), C.c_void_p(d_raw), raw_bytes, C.c_void_p(d_bgzf), bgzf_cap,
                                              C.c_void_p(d_totals), C.c_void_p(d_work), work_bytes))


def bgzf_deflate_work_bytes(raw_bytes: int) -> int:
    return int(hip_lib().pssbam_bgzf_deflate_work_bytes(raw_bytes))


def index_records(buf: np.ndarray) -> np.ndarray:
    """offsets (n+1,) u32 of the whole records in an inflated BAM record stream"""
    L = hip_lib()
    n = L.pssbam_index_records(buf.ctypes.data, buf.size, None, 1 << 62, None)
    if n < 0:
        _chk(int(n))
    offs = np.empty(n + 1, dtype=np.uint32)
    consumed = C.c_uint64()
    n2 = L.pssbam_index_records(buf.ctypes.data, buf.size, offs.ctypes.data, n, C.byref(consumed))
    assert n2 == n
    return offs


@dataclass
class Tables:
    fwd: np.ndarray | None
    rev: np.ndarray | None
    k5: np.ndarray | None
    k3: np.ndarray | None
    stats: dict


class Engine:
    """One engine = one GPU, one stream.  Options mirror the two reference CLIs:
    `pss` = dict(region_len, min_read_len, max_read_len, min_mq, up_ctx, down_ctx, merged_only),
    `kmer` = dict(klen, min_mq, min_read_len, max_read_len, merged_only).
    `read_groups` = @RG IDs (pss-bam -G): one set of substitution tables per ID, see set_read_groups.
    `length_bins` = length bin edges (pss-bam -S): one set of substitution tables per bin, see set_length_bins.
    `contig_sets` = contig sets (pss-bam -C): one set of substitution tables per label, see set_contig_sets.
    `min_base_qual` = minimum base quality (pss-bam -Q): read bases below it are left out of the substitution tables,
    see set_min_base_quality; 0 = off.
    `length_hist` = limit of the fragment-length histogram (pss-bam -H) of the reads added to the substitution tables,
    see set_length_histogram; 0 = off.
    `site_context` = "cpg" (pss-bam -X cpg): a second pair of tables over the positions whose reference site is in CpG
    context, see set_site_context; None = off.
    `end_condition` = (depth, cell5, cell3) (pss-bam -E): a second pair of tables over the unpaired reads whose other end
    carries the given cell within its first `depth` positions, see set_end_condition; None = off.
    `gapped` = True (pss-bam -I): clipped and gapped reads are tallied by their anchored ends, see set_gapped.
    `per_contig` = True (pss-bam -A): every BAM reference's own pair of substitution tables, see set_per_contig.
    `mismatches` = (hist_max, max_mismatches, tv_only) (pss-bam -N / -n / -V): the histogram of, and a filter on, the
    number of mismatches between the whole read and the reference, see set_mismatches; None = off.
    `replicates` = K (pss-bam -J): one set of substitution tables per read-name replicate, the planes of a delete-one-group
    jackknife, see set_replicates; 0 = off.
    `interior` = d (pss-bam -W): the 4 x 4 substitution table of the read interior, the positions at least d bases from both
    ends of every tallied read, see set_interior; None = off.
    `composition` = w (pss-bam -P): the reference base composition w bases on either side of the 5' end of the reads in the
    forward table and of the 3' end of those in the reverse table, see set_composition; None = off.
    `read_score` = dict(weights=, min_score=, hist_half=, hist_shift=) (pss-bam -y / -Y): a filter on, and the histogram of, a
    weighted score over the C and G sites of the whole read, see set_read_score; None = off.
    With `kmer` alone (no `pss`) the three split the k-mer tables instead (fragkon -G / -S / -C): every plane is a
    k5 / k3 pair, and the length bins go by the SEQ length and kmer's min_read_len / max_read_len."""

    def __init__(self, pss: dict | None = None, kmer: dict | None = None, read_group: str | None = None,
                 kernel: int = KERNEL_AUTO, device: int = -1, read_groups: list[str] | None = None,
                 length_bins: list[int] | None = None, contig_sets=None, min_base_qual: int = 0,
                 length_hist: int = 0, site_context: str | None = None, end_condition: tuple[int, int, int] | None = None,
                 gapped: bool = False, per_contig: bool = False, mismatches: tuple[int, int, int] | None = None,
                 replicates: int = 0, interior: int | None = None, composition: int | None = None,
                 read_score: dict | None = None):
        L = hip_lib()
        cfg = _Config()
        cfg.abi_version = 1
        cfg.tally_mask = (TALLY_PSS if pss is not None else 0) | (TALLY_KMER if kmer is not None else 0)
        self._keep = []
        if pss is not None:
            up, dn = pss.get("up_ctx", "ACGT").encode(), pss.get("down_ctx", "ACGT").encode()
            self._keep += [up, dn]
            cfg.pss = _PssOpts(pss.get("region_len", 15), pss.get("min_read_len", 0),
                               pss.get("max_read_len", 250000000), pss.get("min_mq", 0), up, dn,
                               int(pss.get("merged_only", False)))
            self.region_len = cfg.pss.region_len
            self._len_range = (cfg.pss.min_read_len, cfg.pss.max_read_len)
        if kmer is not None:
            cfg.kmer = _KmerOpts(kmer.get("klen", 8), kmer.get("min_mq", 0), kmer.get("min_read_len", 0),
                                 kmer.get("max_read_len", 250000000), int(kmer.get("merged_only", False)))
            self.klen = cfg.kmer.klen
            if pss is None:
                self._len_range = (cfg.kmer.min_read_len, cfg.kmer.max_read_len)
        self.has_pss, self.has_kmer = pss is not None, kmer is not None
        if read_group is not None:
            rg = read_group.encode()
            self._keep.append(rg)
            cfg.read_group = rg
        cfg.device = device
        cfg.kernel = kernel
        h = C.c_void_p()
        _chk(L.pssbam_engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._L = L
        self.read_groups: list[str] = []
        self.length_bins: list[tuple[int, int]] = []
        self.contig_sets: list[str] = []
        self._min_base_qual = 0
        self._length_hist = 0
        self._site_context = SITE_NONE
        if min_base_qual:
            self.set_min_base_quality(min_base_qual)
        if length_hist:
            self.set_length_histogram(length_hist)
        if site_context is not None:
            self.set_site_context(site_context)
        self._end_condition = (0, 0, 0)
        if end_condition is not None:
            self.set_end_condition(*end_condition)
        self._gapped = False
        if gapped:
            self.set_gapped(True)
        self._per_contig = False
        self._n_ref: int | None = None   # the reference count the engine has been told (set_references, feed_open)
        if per_contig:
            self.set_per_contig(True)
        self._mismatches = (0, -1, 0)
        if mismatches is not None:
            self.set_mismatches(*mismatches)
        if read_groups is not None:
            self.set_read_groups(read_groups)
        if length_bins is not None:
            self.set_length_bins(length_bins)
        if contig_sets is not None:
            self.set_contig_sets(contig_sets)
        self._replicates = 0
        if replicates:
            self.set_replicates(replicates)
        self._interior = -1
        if interior is not None:
            self.set_interior(interior)
        self._composition = 0
        if composition is not None:
            self.set_composition(composition)
        self._read_score = None
        if read_score is not None:
            self.set_read_score(**read_score)

    def set_min_base_quality(self, q: int):
        """pss-bam -Q: a read base whose Phred quality is below q (0..93, 0 = off) adds nothing to the substitution
        tables -- the tables equal those of the same records with such bases replaced by N.  Before the first tally
        (after feed_open: before set_references); survives reset."""
        _chk(self._L.pssbam_engine_set_min_base_quality(self._h, int(q)))
        self._min_base_qual = int(q)

    @property
    def min_base_qual(self) -> int:
        """the minimum base quality in force (0 = off)"""
        return self._min_base_qual

    def set_length_histogram(self, max_len: int):
        """pss-bam -H: counts the length (the one -l / -L compare) of every read that is added to the forward / reverse
        table, in the tally kernel itself; lengths above max_len (1..65535, 0 = off) share one last row.  Not with read
        groups, length bins or contig sets.  Before the first tally (after feed_open: before set_references) and before
        bind_counters: the counter block grows by 2 * (max_len + 2) words.  Survives reset."""
        _chk(self._L.pssbam_engine_set_length_histogram(self._h, int(max_len)))
        self._length_hist = int(max_len)

    @property
    def length_hist(self) -> int:
        """the limit of the length histogram in force (0 = off)"""
        return self._length_hist

    def finish_length_hist(self) -> tuple[np.ndarray, np.ndarray]:
        """(fwd, rev): u64 arrays of max_len + 2 rows -- row l = reads of length l added to that table, the last row
        every longer read (drains like finish)"""
        fwd = np.zeros(self._length_hist + 2, dtype=np.uint64)
        rev = np.zeros_like(fwd)
        _chk(self._L.pssbam_engine_finish_length_histogram(self._h, fwd.ctypes.data, rev.ctypes.data))
        return fwd, rev

    def set_site_context(self, mode):
        """pss-bam -X: "cpg" (or SITE_CPG) keeps a second pair of tables, IN, over the interior positions whose reference
        position is in CpG context -- the tables of the same records with every other read base replaced by N; None /
        "none" switches it off.  Not with kmer, read groups, length bins, contig sets or the length histogram.  Before
        the first tally (after feed_open: before set_references) and before bind_counters: the counter block grows by
        2 * (region_len + 2) * 16 words.  Survives reset."""
        if isinstance(mode, str) or mode is None:
            if mode not in SITE_MODES:
                raise ValueError(f"unknown site context {mode!r}")
            mode = SITE_MODES[mode]
        _chk(self._L.pssbam_engine_set_site_context(self._h, int(mode)))
        self._site_context = int(mode)

    @property
    def site_context(self) -> str | None:
        """the site context in force ("cpg" or None)"""
        return "cpg" if self._site_context == SITE_CPG else None

    def finish_site_context(self) -> tuple[np.ndarray, np.ndarray]:
        """(fwd_in, rev_in): the in-context tables, (region_len + 2, 16) u64 each, rows 0 / 1 as in finish() (drains
        like finish); the out-of-context tables are finish() minus these on rows 2+"""
        fwd = np.zeros((self.region_len + 2, 16), dtype=np.uint64)
        rev = np.zeros_like(fwd)
        _chk(self._L.pssbam_engine_finish_site_context(self._h, fwd.ctypes.data, rev.ctypes.data))
        return fwd, rev

    def set_end_condition(self, depth: int, cell5: int = 13, cell3: int = 13):
        """pss-bam -E: keeps a second pair of tables, COND, and four read counters.  An unpaired read is 5'-marked when one
        of the first `depth` (1..MAX_END_DEPTH, <= region_len) positions of its 5' end carries cell `cell5`
        (4 * read base + reference base, A C G T = 0..3, in read orientation; 13 = C->T, 2 = G->A) and 3'-marked likewise
        with `cell3` at its 3' end; COND's forward table holds the 3'-marked reads, its reverse table the 5'-marked ones.
        depth 0 switches it off.  Needs region_len <= 30; not with kmer, read groups, length bins, contig sets, the length
        histogram or site context.  Before the first tally (after feed_open: before set_references) and before
        bind_counters: the counter block grows by 2 * (region_len + 2) * 16 + 4 words.  Survives reset."""
        _chk(self._L.pssbam_engine_set_end_condition(self._h, int(depth), int(cell5), int(cell3)))
        self._end_condition = (int(depth), int(cell5), int(cell3)) if depth else (0, 0, 0)

    @property
    def end_condition(self) -> tuple[int, int, int] | None:
        """the end condition in force, (depth, cell5, cell3), or None"""
        return self._end_condition if self._end_condition[0] else None

    def finish_end_condition(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(fwd_c, rev_c, reads): the conditional tables, (region_len + 2, 16) u64 each, and reads[4] = unpaired reads
        added to the tables, the 5'-marked, the 3'-marked and the both-marked ones among them (drains like finish)"""
        fwd = np.zeros((self.region_len + 2, 16), dtype=np.uint64)
        rev = np.zeros_like(fwd)
        reads = np.zeros(4, dtype=np.uint64)
        _chk(self._L.pssbam_engine_finish_end_condition(self._h, fwd.ctypes.data, rev.ctypes.data, reads.ctypes.data))
        return fwd, rev, reads

    def set_gapped(self, on: bool):
        """pss-bam -I: a read whose CIGAR is [H][S] core [S][H] with a core of M I D = X ops that starts and ends with a
        match-type op (and whose query lengths add up to its SEQ) is tallied by its anchored ends -- as the record
        <span>M whose SEQ keeps the match-type run at either end of the core and holds N in between, so a position
        between two indels adds nothing; every other record is treated as before.  Not with kmer, read groups, length bins, contig
        sets, the length histogram, site context or the end condition.  Before the first tally (after feed_open: before
        set_references); the counter block does not change.  Survives reset."""
        _chk(self._L.pssbam_engine_set_gapped_reads(self._h, int(bool(on))))
        self._gapped = bool(on)

    @property
    def gapped(self) -> bool:
        """whether clipped and gapped reads are tallied by their anchored ends"""
        return self._gapped

    def set_mismatches(self, hist_max: int = 0, max_mismatches: int = -1, tv_only: int = 0):
        """pss-bam -N / -n / -V.  m = the positions of a <L>M read at which read and reference base are both A/C/G/T and
        differ (tv_only: differ by a transversion).  max_mismatches = k (0..255, -1 = off): a read that would be tallied
        and has m > k is filtered instead -- the tables are those of the input without such reads.  hist_max = M (1..255,
        0 = off): counts min(m, M + 1) of every read that is added to the forward / reverse table, see
        finish_mismatches.  (0, -1, x) switches both off.  Needs region_len <= 30; goes with read_group, min_base_qual
        and regions; not with kmer, read groups, length bins, contig sets, per-contig tables, the length histogram, site
        context, the end condition or gapped reads.  Before the first tally (after feed_open: before set_references);
        a histogram also before bind_counters: the counter block grows by 2 * (hist_max + 2) words.  Survives reset."""
        _chk(self._L.pssbam_engine_set_mismatches(self._h, int(hist_max), int(max_mismatches), int(bool(tv_only))))
        on = hist_max > 0 or max_mismatches >= 0
        self._mismatches = (int(hist_max), int(max_mismatches), int(bool(tv_only)) if on else 0)

    @property
    def mismatches(self) -> tuple[int, int, int] | None:
        """(hist_max, max_mismatches, tv_only) in force, None = off"""
        return self._mismatches if self._mismatches[0] > 0 or self._mismatches[1] >= 0 else None

    def finish_mismatches(self) -> tuple[np.ndarray, np.ndarray]:
        """(fwd, rev): u64 arrays of hist_max + 2 rows -- row m = reads with m mismatches added to that table, the last
        row every larger count (drains like finish)"""
        fwd = np.zeros(self._mismatches[0] + 2, dtype=np.uint64)
        rev = np.zeros_like(fwd)
        _chk(self._L.pssbam_engine_finish_mismatches(self._h, fwd.ctypes.data, rev.ctypes.data))
        return fwd, rev

    def set_per_contig(self, on: bool = True):
        """pss-bam -A: plane k of the counter block takes the records whose refID is k (k = 0 .. n_ref - 1 of
        set_references; plane n_ref: refID -1) -- what the ordinary tables receive from them, so the tables of a run
        on the genome reduced to that contig -- for any number of references, in one pass.  finish() stays the total,
        finish_contigs() returns the planes.  Goes with read_group, min_base_qual and regions; not with kmer, read
        groups, length bins, contig sets, the length histogram, site context, the end condition or gapped reads.
        Before the first tally (after feed_open: before set_references) and before bind_counters: the block is sized
        for n_ref + 1 planes when the reference count is known.  Survives reset."""
        _chk(self._L.pssbam_engine_set_per_contig(self._h, int(bool(on))))
        self._per_contig = bool(on)

    @property
    def per_contig(self) -> bool:
        """whether every BAM reference has its own pair of tables"""
        return self._per_contig

    def finish_contigs(self, first: int = 0, n: int | None = None) -> dict:
        """{refID: Tables} of the planes among first .. first + n - 1 (default: all) that hold something; the refID -1
        records are under key n_ref (drains like finish).  Only the touched planes are read back from the device."""
        if n is None:
            n = (self._n_ref or 0) + 1 - first
        cells = (self.region_len + 2) * 16
        touched = np.zeros(max(n, 1), dtype=np.uint8)
        _chk(self._L.pssbam_engine_finish_contigs(self._h, first, n, None, None, touched.ctypes.data))
        out = {}
        hit = np.flatnonzero(touched[:n])
        # runs of touched neighbours, one call each
        for run in np.split(hit, np.flatnonzero(np.diff(hit) != 1) + 1) if hit.size else []:
            fwd = np.zeros((run.size, self.region_len + 2, 16), dtype=np.uint64)
            rev = np.zeros_like(fwd)
            assert fwd.size == run.size * cells
            _chk(self._L.pssbam_engine_finish_contigs(self._h, first + int(run[0]), int(run.size), fwd.ctypes.data, rev.ctypes.data, None))
            for i, k in enumerate(run):
                out[first + int(k)] = Tables(fwd[i], rev[i], None, None, {})
        return out

    def set_regions(self, names, name_of, starts, ends):
        """pss-bam -T / fragkon -T: only records whose alignment overlaps one of the intervals are tallied -- the tables
        equal those of the input reduced by `samtools view -L`.  Interval i is the 0-based half-open
        [starts[i], ends[i]) on contig names[name_of[i]] (numpy arrays or sequences; any order, may overlap).  No
        interval switches the filter off.  Before the first tally (after feed_open: before set_references), before or
        after set_references; survives reset."""
        raw = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm in names]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        name_of = np.ascontiguousarray(name_of, dtype=np.int32)
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        ends = np.ascontiguousarray(ends, dtype=np.uint32)
        if not (name_of.size == starts.size == ends.size):
            raise ValueError("name_of, starts and ends must have one entry per interval")
        _chk(self._L.pssbam_engine_set_regions(self._h, len(raw), arr, name_of.size, name_of.ctypes.data, starts.ctypes.data,
                                               ends.ctypes.data))

    def set_contig_sets(self, sets):
        """pss-bam -C: tallies every record into the tables of the set that lists its RNAME (the unassigned bucket
        otherwise).  `sets` = {label: [contig names]} or [(contig name, label)]; labels are numbered in order of
        first appearance.  Before the first tally, like set_read_groups; before or after set_references."""
        pairs = [(nm, lab) for lab, nms in sets.items() for nm in nms] if isinstance(sets, dict) else list(sets)
        labels: list[str] = []
        index: dict[str, int] = {}
        for _, lab in pairs:
            if lab not in index:
                index[lab] = len(labels)
                labels.append(lab)
        names = (C.c_char_p * max(len(pairs), 1))(*[nm.encode() if isinstance(nm, str) else bytes(nm) for nm, _ in pairs])
        set_of = (C.c_int32 * max(len(pairs), 1))(*[index[lab] for _, lab in pairs])
        _chk(self._L.pssbam_engine_set_contig_sets(self._h, len(labels), len(pairs), names, set_of))
        self.contig_sets = labels

    def finish_sets(self) -> dict:
        """{label: Tables} per contig set, in set order (fwd / rev, or k5 / k3 on a k-mer engine; drains like finish)"""
        return self._finish_planes(enumerate(self.contig_sets))

    def set_length_bins(self, edges: list[int]):
        """pss-bam -S: tallies every record into the tables of its length bin [min_read_len, e1-1], [e1, e2-1], ...,
        [ek, max_read_len] (the length -l / -L compare).  Before the first tally, like set_read_groups."""
        edges = [int(x) for x in edges]
        arr = (C.c_uint32 * max(len(edges), 1))(*[x & 0xFFFFFFFF for x in edges])
        _chk(self._L.pssbam_engine_set_length_bins(self._h, len(edges), arr))
        lo, hi = self._len_range
        starts, ends = [lo] + edges, [x - 1 for x in edges] + [hi]
        self.length_bins = list(zip(starts, ends))

    def set_interior(self, margin: int = -1):
        """pss-bam -W.  margin = d (0..65535, -1 = off): every record that is added to the forward or the reverse table also
        counts its interior positions i (d <= i, i + d < L, i < l_seq) at which read and reference base are both A/C/G/T --
        and, with min_base_qual, QUAL[i] is not below it -- into a 4 x 4 table, bin 4 * read + ref, a reverse-strand read into
        15 - that; see finish_interior.  d = 0 is the whole read.  Needs region_len <= 30; goes with read_group, min_base_qual
        and regions; not with kmer, read groups, length bins, contig sets, per-contig tables, replicates, the length
        histogram, site context, the end condition, gapped reads or the mismatch count.  Before the first tally (after
        feed_open: before set_references) and before bind_counters: the counter block grows by 17 words.  Survives reset."""
        _chk(self._L.pssbam_engine_set_interior(self._h, int(margin)))
        self._interior = int(margin)

    @property
    def interior(self) -> int | None:
        """the interior margin in force, None = off"""
        return self._interior if self._interior >= 0 else None

    def finish_interior(self) -> tuple[np.ndarray, int]:
        """(table, reads): table = u64[16], bin 4 * read + ref (A C G T) in the read's orientation; reads = the tallied
        records whose interior is not empty (drains like finish)"""
        table = np.zeros(16, dtype=np.uint64)
        reads = np.zeros(1, dtype=np.uint64)
        _chk(self._L.pssbam_engine_finish_interior(self._h, table.ctypes.data, reads.ctypes.data))
        return table, int(reads[0])

    def set_read_score(self, weights=None, min_score: int | None = None, hist_half: int = 0, hist_shift: int = 0):
        """pss-bam -y / -Y.  weights: integers [4][n_dist][n_qual] (n_dist, n_qual 1..64, |w| <= 2047), None = off.  The score S
        of a <L>M read sums weights[kind][d][q] over the positions where read and reference are both A/C/G/T (and QUAL passes
        min_base_qual): reference C under read C / T is kind 0 / 1 at d = i, reference G under read G / A kind 2 / 3 at
        d = L-1-i, a reverse-strand read swaps 0 1 with 2 3; d and q = QUAL[i] saturate at the last row / column.  min_score
        (None = no filter): a read that would be tallied and has S < min_score is filtered instead.  hist_half = H (1..128,
        0 = off): counts bin clamp(S >> hist_shift, -H, H-1) + H of every read added to the forward / reverse table, see
        finish_read_score.  Needs region_len <= 30; goes with read_group, min_base_qual and regions; not with kmer, any
        plane split, the length histogram, site context, the end condition, gapped reads, the mismatch count, the interior
        or the composition table.  Before the first tally (after feed_open: before set_references); a histogram also before
        bind_counters: the counter block grows by 4 * hist_half words.  Survives reset."""
        if weights is None:
            _chk(self._L.pssbam_engine_set_read_score(self._h, None, 0, 0, 0, 0, 0, 0))
            self._read_score = None
            return
        w = np.asarray(weights)
        if w.ndim != 3 or w.shape[0] != 4:
            raise PssbamError("read-score weights must have the shape [4][n_dist][n_qual]")
        if w.size and (np.abs(w.astype(np.int64)) > 32767).any():
            raise PssbamError("read-score weights must fit 16 bits")
        w16 = np.ascontiguousarray(w, dtype=np.int16)
        _chk(self._L.pssbam_engine_set_read_score(self._h, w16.ctypes.data, w.shape[1], w.shape[2], int(min_score is not None),
                                                  int(min_score or 0), int(hist_half), int(hist_shift)))
        self._read_score = dict(weights=w16, min_score=None if min_score is None else int(min_score), hist_half=int(hist_half),
                                hist_shift=int(hist_shift))

    @property
    def read_score(self) -> dict | None:
        """the read-score setting in force (weights, min_score, hist_half, hist_shift), None = off"""
        return self._read_score

    def finish_read_score(self) -> tuple[np.ndarray, np.ndarray]:
        """(fwd, rev): u64 arrays of 2 * hist_half rows -- row b = reads of score bin b - hist_half added to that table, the
        first and last row everything below / above (drains like finish)"""
        if not self._read_score or not self._read_score["hist_half"]:
            raise PssbamError("set_read_score has not been called with a histogram")
        fwd = np.zeros(2 * self._read_score["hist_half"], dtype=np.uint64)
        rev = np.zeros_like(fwd)
        _chk(self._L.pssbam_engine_finish_read_score(self._h, fwd.ctypes.data, rev.ctypes.data))
        return fwd, rev

    def set_composition(self, width: int = 0):
        """pss-bam -P.  width = w (1..MAX_COMPOSITION, 0 = off): every record that is added to the forward table counts the
        reference bases at the offsets -w .. w-1 from its 5' end (negative: outside the read), every record that is added to
        the reverse table those around its 3' end, in the read's orientation, as A C G T or other; see finish_composition.
        Positions outside the contig, and inside offsets at or beyond the read's length, count nothing.  Needs
        region_len <= 30; goes with read_group, min_base_qual (no effect) and regions; not with kmer, read groups, length
        bins, contig sets, per-contig tables, replicates, the length histogram, site context, the end condition, gapped
        reads, the mismatch count or the interior table.  Before the first tally (after feed_open: before set_references)
        and before bind_counters: the counter block grows by 20 * w words.  Survives reset."""
        _chk(self._L.pssbam_engine_set_composition(self._h, int(width)))
        self._composition = int(width)

    @property
    def composition(self) -> int | None:
        """the composition width in force, None = off"""
        return self._composition if self._composition > 0 else None

    def finish_composition(self) -> tuple[np.ndarray, np.ndarray]:
        """(c5, c3): u64 arrays of shape (2w, 5), row j + w = offset j from the 5' / 3' end, columns A C G T other
        (drains like finish)"""
        if not self._composition:
            raise PssbamError("set_composition has not been called with a width")
        c5 = np.zeros((2 * self._composition, 5), dtype=np.uint64)
        c3 = np.zeros((2 * self._composition, 5), dtype=np.uint64)
        _chk(self._L.pssbam_engine_finish_composition(self._h, c5.ctypes.data, c3.ctypes.data))
        return c5, c3

    def set_replicates(self, k: int):
        """pss-bam -J: tallies every record into the tables of its replicate among k (2..MAX_REPLICATES; 0 switches it
        off), picked by a hash of its read name (include/pssbam_hip.h), so mates share one: replicate j holds what the
        same engine tallies on the input reduced to its records.  finish() stays the total, finish_replicates()
        returns the planes.  Goes with read_group, min_base_qual and regions; not with kmer, read groups, length bins,
        contig sets, per-contig tables, the length histogram, site context, the end condition, gapped reads or the
        mismatch count.  Before the first tally (after feed_open: before set_references) and before bind_counters: the
        counter block grows by k * 2 * (region_len + 2) * 16 words.  Survives reset."""
        _chk(self._L.pssbam_engine_set_replicates(self._h, int(k)))
        self._replicates = int(k)

    @property
    def replicates(self) -> int:
        """the number of read-name replicates in force (0 = off)"""
        return self._replicates

    def finish_replicates(self) -> tuple[np.ndarray, np.ndarray]:
        """(fwd, rev): the replicates' tables stacked, (k, region_len + 2, 16) u64 each (drains like finish)"""
        if not self._replicates:
            raise PssbamError("set_replicates has not been called")
        planes = self._finish_planes(enumerate(range(self._replicates)))
        fwd = np.stack([planes[j].fwd for j in range(self._replicates)])
        rev = np.stack([planes[j].rev for j in range(self._replicates)])
        return fwd, rev

    def set_read_groups(self, ids: list[str]):
        """pss-bam -G: tallies every record into the tables of the ID its first RG:Z value equals (the unassigned
        bucket otherwise).  Before the first tally (after feed_open: before set_references)."""
        raw = [i.encode() if isinstance(i, str) else bytes(i) for i in ids]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        _chk(self._L.pssbam_engine_set_read_groups(self._h, len(raw), arr))
        self.read_groups = [i.decode() if isinstance(i, bytes) else i for i in ids]

    def finish_groups(self) -> dict:
        """{ID: Tables, ..., None: Tables of the unassigned bucket} (fwd / rev, or k5 / k3 on a k-mer engine; drains
        like finish)"""
        return self._finish_planes([(-1, None)] + list(enumerate(self.read_groups)))

    def finish_bins(self) -> dict:
        """{(lo, hi): Tables} per length bin (fwd / rev, or k5 / k3 on a k-mer engine; drains like finish)"""
        return self._finish_planes(enumerate(self.length_bins))

    def _finish_planes(self, planes) -> dict:
        """{key: Tables} for (plane, key) pairs of pssbam_engine_finish_groups; a repeated key keeps its first plane"""
        out = {}
        for g, key in planes:
            if not self.has_pss:   # k-mer planes
                k5 = np.zeros(4 ** self.klen, dtype=np.uint64)
                k3 = np.zeros_like(k5)
                _chk(self._L.pssbam_engine_finish_kmer_groups(self._h, g, k5.ctypes.data, k3.ctypes.data))
                if key not in out:
                    out[key] = Tables(None, None, k5, k3, {})
                continue
            fwd = np.zeros((self.region_len + 2, 16), dtype=np.uint64)
            rev = np.zeros_like(fwd)
            _chk(self._L.pssbam_engine_finish_groups(self._h, g, fwd.ctypes.data, rev.ctypes.data))
            if key not in out:   # a repeated ID: its first index holds the counts
                out[key] = Tables(fwd, rev, None, None, {})
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.pssbam_engine_destroy(self._h)
            self._h = None

    __del__ = close

    def set_record_sink(self, sink="collect"):
        """The record sink (pssbam_engine_set_record_sink): the engine hands over the records it added to the forward or the
        reverse table, byte-identical and in input order.  sink = "collect": the chunks are kept and finish_records() returns
        them as one uint8 array; a callable f(chunk: uint8 array, n_records) -> int | None is called per chunk (a non-zero
        return fails the engine call, and the sink is not called again); None: off.  Before the first submit."""
        self._sink_chunks, self._sink_records = [], 0
        if sink is None:
            self._sink_cb = None
            _chk(self._L.pssbam_engine_set_record_sink(self._h, None, None))
            return
        collect = sink == "collect"

        def cb(_ctx, ptr, nbytes, n_records):
            chunk = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(int(nbytes),)).copy()   # (valid during the call only)
            if collect:
                self._sink_chunks.append(chunk)
                self._sink_records += int(n_records)
                return 0
            try:
                return int(sink(chunk, int(n_records)) or 0)
            except Exception:   # (an exception cannot cross the C frames)
                return 1

        self._sink_cb = _RECORD_SINK(cb)   # (kept alive with the engine)
        _chk(self._L.pssbam_engine_set_record_sink(self._h, self._sink_cb, None))

    def set_block_sink(self, sink="collect"):
        """The block sink (pssbam_engine_set_block_sink): the record sink's stream as whole BGZF blocks, deflated on the
        device.  sink = "collect": the chunks are kept and finish_blocks() returns them as one uint8 array; a callable
        f(blocks: uint8 array, n_blocks, raw_bytes, n_records) -> int | None is called per chunk (a non-zero return fails the
        engine call, and the sink is not called again); None: off.  Before the first submit; not beside a record sink."""
        self._block_chunks, self._block_totals = [], [0, 0, 0]
        if sink is None:
            self._block_cb = None
            _chk(self._L.pssbam_engine_set_block_sink(self._h, None, None))
            return
        collect = sink == "collect"

        def cb(_ctx, ptr, nbytes, n_blocks, raw_bytes, n_records):
            chunk = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(int(nbytes),)).copy()   # (valid during the call only)
            if collect:
                self._block_chunks.append(chunk)
                for k, v in enumerate((n_blocks, raw_bytes, n_records)):
                    self._block_totals[k] += int(v)
                return 0
            try:
                return int(sink(chunk, int(n_blocks), int(raw_bytes), int(n_records)) or 0)
            except Exception:   # (an exception cannot cross the C frames)
                return 1

        cb_c = _BLOCK_SINK(cb)
        _chk(self._L.pssbam_engine_set_block_sink(self._h, cb_c, None))
        self._block_cb = cb_c   # (kept alive with the engine)

    def set_end_mask(self, mode, n5, n3=None):
        """The end mask (pssbam_engine_set_end_mask): the first n5 bases of the 5' end and the first n3 (default: n5) of the 3'
        end of every record a sink receives become N with quality 0 -- mode "all": every base there; "ds": T at the 5' and A
        at the 3' end, in the read's orientation; "ss": T at both; None, "off" or 0: off.  The tables do not change.  Before
        the first submit."""
        m = END_MASK_MODES[mode] if mode is None or isinstance(mode, str) else int(mode)
        _chk(self._L.pssbam_engine_set_end_mask(self._h, m, int(n5), int(n5 if n3 is None else n3)))

    def set_duplicates(self, on: bool = True, initial_slots: int = 0):
        """Duplicate flagging (pssbam_engine_set_duplicates): the engine sets FLAG 0x400 of every eligible unpaired record that an
        earlier one, in input order, shares (refID, POS, SEQ length, strand, read-group plane) with, in its device copy and in front
        of the tally.  initial_slots: the key table's first size (0 = the default; it doubles as needed).  Before the first submit;
        not with set_gapped, not on an engine with both tallies."""
        _chk(self._L.pssbam_engine_set_duplicates(self._h, 1 if on else 0, int(initial_slots)))

    def finish_duplicates(self, hist_max: int = 255) -> tuple[dict, np.ndarray]:
        """sync, then ({"eligible", "distinct", "flagged"}, hist): hist[c] = the keys with exactly c eligible records for c in
        1..hist_max, hist[hist_max + 1] the keys with more"""
        totals = np.zeros(3, dtype=np.uint64)
        hist = np.zeros(int(hist_max) + 2, dtype=np.uint64)
        _chk(self._L.pssbam_engine_finish_duplicates(self._h, totals.ctypes.data, hist.ctypes.data, int(hist_max)))
        return dict(zip(("eligible", "distinct", "flagged"), (int(v) for v in totals))), hist

    def set_coverage(self, on: bool = True, positions_hint: int = 0):
        """Depth of coverage of the kept records (pssbam_engine_set_coverage): one uint32 per stored genome position, two atomic
        adds per kept record behind each block's tally.  positions_hint: the genome's expected positions, for the feed's memory
        budget.  Before the first submit; needs the substitution tally; not with set_gapped."""
        _chk(self._L.pssbam_engine_set_coverage(self._h, 1 if on else 0, int(positions_hint)))

    def finish_coverage(self, n_ref: int, hist_max: int = COV_HIST_MAX) -> tuple[np.ndarray, np.ndarray, int]:
        """sync, then (per_contig, hist, n_runs) of everything since create / reset: per_contig[i] = {covered, depth_sum, max_depth}
        of reference i in 0..n_ref-1, hist[d] = the positions at depth d for d in 0..hist_max and hist[hist_max + 1] those above.
        Non-destructive."""
        per = np.zeros((int(n_ref), 3), dtype=np.uint64)
        hist = np.zeros(int(hist_max) + 2, dtype=np.uint64)
        n_runs = C.c_uint64(0)
        _chk(self._L.pssbam_engine_finish_coverage(self._h, 0, int(n_ref), per.ctypes.data if n_ref else None, hist.ctypes.data, int(hist_max),
                                                   C.addressof(n_runs)))
        return per, hist, int(n_runs.value)

    def finish_coverage_runs(self, cap: int | None = None, count_only: bool = False):
        """sync, then the covered intervals as (ref, start, end, depth) arrays -- half-open, by refID then start -- or, with
        count_only, their number.  cap: the room to offer (default: the exact count, asked for first)."""
        n_runs = C.c_uint64(0)
        if count_only or cap is None:
            _chk(self._L.pssbam_engine_finish_coverage_runs(self._h, 0, None, None, None, None, C.addressof(n_runs)))
            if count_only:
                return int(n_runs.value)
            cap = int(n_runs.value)
        ref = np.zeros(max(int(cap), 1), dtype=np.int32)
        start, end, depth = (np.zeros(max(int(cap), 1), dtype=np.uint32) for _ in range(3))
        _chk(self._L.pssbam_engine_finish_coverage_runs(self._h, int(cap), ref.ctypes.data, start.ctypes.data, end.ctypes.data, depth.ctypes.data,
                                                        C.addressof(n_runs)))
        n = int(n_runs.value)
        return ref[:n], start[:n], end[:n], depth[:n]

    def finish_coverage_windows(self, window: int, cap: int | None = None, count_only: bool = False):
        """sync, then the fixed windows of `window` positions (16 .. 2**30) of every reference the genome holds as (ref, start, end,
        acgt, gc, covered, depth_sum) arrays -- half-open, by refID then start, the last window of a contig possibly short -- or,
        with count_only, their number.  cap: the room to offer (default: the exact count, asked for first).  Non-destructive."""
        n_win = C.c_uint64(0)
        if count_only or cap is None:
            _chk(self._L.pssbam_engine_finish_coverage_windows(self._h, int(window), 0, None, None, None, None, None, None, None, C.addressof(n_win)))
            if count_only:
                return int(n_win.value)
            cap = int(n_win.value)
        ref = np.zeros(max(int(cap), 1), dtype=np.int32)
        start, end, acgt, gc, covered = (np.zeros(max(int(cap), 1), dtype=np.uint32) for _ in range(5))
        depth_sum = np.zeros(max(int(cap), 1), dtype=np.uint64)
        _chk(self._L.pssbam_engine_finish_coverage_windows(self._h, int(window), int(cap), ref.ctypes.data, start.ctypes.data, end.ctypes.data,
                                                           acgt.ctypes.data, gc.ctypes.data, covered.ctypes.data, depth_sum.ctypes.data,
                                                           C.addressof(n_win)))
        n = int(n_win.value)
        return ref[:n], start[:n], end[:n], acgt[:n], gc[:n], covered[:n], depth_sum[:n]

    def set_sites(self, names, name_of, pos0, trim: int = 0):
        """Strand-split allele counts of the kept records at listed sites (pssbam_engine_set_sites): site i is the 0-based position
        pos0[i] on contig names[name_of[i]] (numpy arrays or sequences; any order, duplicates merge); a kept read counts at the sites
        between its first and last `trim` bases.  No site switches it off.  Before the first submit, before or after
        set_references; needs the substitution tally; not with set_gapped; survives reset."""
        raw = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm in names]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        name_of = np.ascontiguousarray(name_of, dtype=np.int32)
        pos0 = np.ascontiguousarray(pos0, dtype=np.uint32)
        if name_of.size != pos0.size:
            raise ValueError("name_of and pos0 must have one entry per site")
        _chk(self._L.pssbam_engine_set_sites(self._h, len(raw), arr, name_of.size, name_of.ctypes.data, pos0.ctypes.data, int(trim)))

    def finish_sites(self, cap: int | None = None):
        """sync, then (ref, pos0, ref_base, counts, totals) of everything since create / reset: the resolved sites by refID then
        position, ref_base as uint8 letters, counts[n, 10] = fA fC fG fT fO rA rC rG rT rO, totals = {"given", "resolved", "covered",
        "bases"}.  Non-destructive.  cap: the room to offer (default: the exact count, asked for first)."""
        n_sites = C.c_uint64(0)
        if cap is None:
            _chk(self._L.pssbam_engine_finish_sites(self._h, 0, None, None, None, None, C.addressof(n_sites), None))
            cap = int(n_sites.value)
        room = max(int(cap), 1)
        ref = np.zeros(room, dtype=np.int32)
        pos0 = np.zeros(room, dtype=np.uint32)
        base = np.zeros(room, dtype=np.uint8)
        counts = np.zeros((room, 10), dtype=np.uint32)
        totals = np.zeros(4, dtype=np.uint64)
        _chk(self._L.pssbam_engine_finish_sites(self._h, int(cap), ref.ctypes.data, pos0.ctypes.data, base.ctypes.data, counts.ctypes.data,
                                                C.addressof(n_sites), totals.ctypes.data))
        n = int(n_sites.value)
        return ref[:n], pos0[:n], base[:n], counts[:n], dict(zip(("given", "resolved", "covered", "bases"), (int(v) for v in totals)))

    def finish_blocks(self) -> np.ndarray:
        """sync, then every block collected since set_block_sink() / the last finish_blocks(), as one uint8 array;
        blocks_kept = {"n_blocks", "raw_bytes", "n_records"} of them"""
        self.sync()
        out = np.concatenate(self._block_chunks) if self._block_chunks else np.zeros(0, dtype=np.uint8)
        self.blocks_kept = dict(zip(("n_blocks", "raw_bytes", "n_records"), self._block_totals))
        self._block_chunks, self._block_totals = [], [0, 0, 0]
        return out

    def finish_records(self) -> np.ndarray:
        """sync, then every record collected since set_record_sink() / the last finish_records(), as one uint8 array"""
        self.sync()
        out = np.concatenate(self._sink_chunks) if self._sink_chunks else np.zeros(0, dtype=np.uint8)
        self.records_kept = self._sink_records
        self._sink_chunks, self._sink_records = [], 0
        return out

    def set_stream(self, hip_stream: int):
        _chk(self._L.pssbam_engine_set_stream(self._h, C.c_void_p(hip_stream)))

    def set_genome_arrays(self, contigs: list[tuple[str, np.ndarray]]):
        """contigs: [(id, uint8 array in loaded form)] (host memory)"""
        n = len(contigs)
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for _, a in contigs]
        ids = (C.c_char_p * n)(*[c[0].encode() for c in contigs])
        seqs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        lens = (C.c_uint64 * n)(*[a.size for a in arrs])
        _chk(self._L.pssbam_engine_set_genome_arrays(self._h, n, ids, seqs, lens, 0))

    def set_genome_device(self, contigs: list[tuple[str, int, int]]):
        """contigs: [(id, device_ptr, length)]"""
        n = len(contigs)
        ids = (C.c_char_p * n)(*[c[0].encode() for c in contigs])
        seqs = (C.c_void_p * n)(*[c[1] for c in contigs])
        lens = (C.c_uint64 * n)(*[c[2] for c in contigs])
        _chk(self._L.pssbam_engine_set_genome_arrays(self._h, n, ids, seqs, lens, 1))

    def set_genome_struct(self, genome_ptr: int):
        """genome_ptr: a Genome* from init_genome (libpssbam_host.so)"""
        _chk(self._L.pssbam_engine_set_genome(self._h, C.c_void_p(genome_ptr)))

    def set_references(self, names: list[str]):
        n = len(names)
        arr = (C.c_char_p * max(n, 1))(*[s.encode() for s in names])
        _chk(self._L.pssbam_engine_set_references(self._h, n, arr))
        self._n_ref = n

    def submit(self, records: np.ndarray, offsets: np.ndarray | None = None):
        records = np.ascontiguousarray(records, dtype=np.uint8)
        if offsets is None:
            offsets = index_records(records)
            if int(offsets[-1]) != records.size:
                raise PssbamError("record block ends in a partial record")
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        _chk(self._L.pssbam_engine_submit(self._h, records.ctypes.data, records.size, offsets.ctypes.data,
                                          offsets.size - 1))

    def submit_async(self, records: np.ndarray, offsets: np.ndarray) -> int:
        """enqueue only; the arrays must stay alive and untouched until wait_copied(ticket)"""
        t = C.c_uint64()
        _chk(self._L.pssbam_engine_submit_async(self._h, records.ctypes.data, records.size, offsets.ctypes.data,
                                                offsets.size - 1, C.byref(t)))
        return int(t.value)

    def wait_copied(self, ticket: int):
        _chk(self._L.pssbam_engine_wait_copied(self._h, ticket))

    def copy_done(self, ticket: int) -> bool:
        rc = self._L.pssbam_engine_copy_done(self._h, ticket)
        if rc < 0:
            _chk(rc)
        return bool(rc)

    def phase_times(self) -> dict:
        a, b, c, d = C.c_double(), C.c_uint64(), C.c_double(), C.c_uint64()
        _chk(self._L.pssbam_engine_phase_times(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"h2d_ms": a.value, "h2d_bytes": b.value, "kernel_ms": c.value, "launches": d.value}

    def feed_open(self, n_ref: int, genome_bytes_hint: int = 0):
        """compressed blocks may be fed before set_genome / set_references; their tallies follow then"""
        self._L.pssbam_engine_feed_open.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
        _chk(self._L.pssbam_engine_feed_open(self._h, n_ref, genome_bytes_hint))
        if self._n_ref is None:
            self._n_ref = n_ref

    def submit_bgzf(self, bgzf: np.ndarray, header_bytes: int = 0, max_batch_inflated: int = 1 << 30, on_busy=None) -> int:
        """Whole BGZF blocks (host bytes) through the device-side feed: inflate, CRC, record index and
        tally on the GPU.  header_bytes = inflated bytes in front of the first alignment record (the BAM
        header when `bgzf` starts at the beginning of the file).  Returns the number of blocks.
        on_busy: called when the engine answers PSSBAM_EBUSY (fed ahead of the genome, every slot full); it
        must set the genome and references, after which the chunk is submitted again."""
        class _Blk(C.Structure):
            _fields_ = [("in_off", C.c_uint64), ("in_len", C.c_uint32), ("isize", C.c_uint32), ("out_off", C.c_uint64),
                        ("crc", C.c_uint32), ("status", C.c_uint32)]
        L = self._L
        L.pssbam_bgzf_scan.restype = C.c_int64
        L.pssbam_bgzf_scan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.pssbam_engine_submit_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32,
                                                C.POINTER(C.c_uint64)]
        L.pssbam_engine_wait_bgzf_copied.argtypes = [C.c_void_p, C.c_uint64]
        bgzf = np.ascontiguousarray(bgzf, dtype=np.uint8)
        consumed = C.c_uint64()
        n = L.pssbam_bgzf_scan(bgzf.ctypes.data, bgzf.size, None, 0, C.byref(consumed), None)
        if n < 0:
            _chk(int(n))
        if consumed.value != bgzf.size:
            raise PssbamError("input ends inside a BGZF block")
        blocks = (_Blk * max(int(n), 1))()
        L.pssbam_bgzf_scan(bgzf.ctypes.data, bgzf.size, blocks, n, None, None)
        i, skip = 0, header_bytes
        while i < n and skip >= blocks[i].isize and (skip > 0 or blocks[i].isize == 0):   # blocks that are all header
            skip -= blocks[i].isize
            i += 1
        while i < n:
            j, base_in, base_out = i, blocks[i].in_off & ~3, blocks[i].out_off
            while j < n and blocks[j].out_off + blocks[j].isize - base_out <= max_batch_inflated:
                j += 1
            j = max(j, i + 1)
            grp = (_Blk * (j - i))()
            for k in range(i, j):
                grp[k - i] = blocks[k]
                grp[k - i].in_off -= base_in
                grp[k - i].out_off -= base_out
            end_in = blocks[j - 1].in_off + blocks[j - 1].in_len
            t = C.c_uint64()
            rc = L.pssbam_engine_submit_bgzf(self._h, bgzf.ctypes.data + base_in, end_in - base_in, grp, j - i, skip, C.byref(t))
            if rc == EBUSY and on_busy is not None:
                on_busy()
                rc = L.pssbam_engine_submit_bgzf(self._h, bgzf.ctypes.data + base_in, end_in - base_in, grp, j - i, skip, C.byref(t))
            _chk(rc)
            _chk(L.pssbam_engine_wait_bgzf_copied(self._h, t.value))
            skip = 0
            i = j
        return int(n)

    def feed_break(self):
        self._L.pssbam_engine_feed_break.argtypes = [C.c_void_p]
        _chk(self._L.pssbam_engine_feed_break(self._h))

    def feed_handoff(self, to: "Engine"):
        """the blocks submitted to `to` from now on continue this engine's stream (include/pssbam_hip.h)"""
        self._L.pssbam_engine_feed_handoff.argtypes = [C.c_void_p, C.c_void_p]
        _chk(self._L.pssbam_engine_feed_handoff(self._h, to._h))

    def feed_status(self) -> dict:
        L = self._L
        L.pssbam_engine_feed_status.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        f, ms, nb = C.c_uint32(), C.c_double(), C.c_uint64()
        _chk(L.pssbam_engine_feed_status(self._h, C.byref(f), C.byref(ms), C.byref(nb)))
        return {"flags": int(f.value), "inflate_ms": float(ms.value), "inflated_bytes": int(nb.value)}

    def submit_device(self, d_records: int, nbytes: int, d_offsets: int, n_records: int):
        _chk(self._L.pssbam_engine_submit_device(self._h, C.c_void_p(d_records), nbytes, C.c_void_p(d_offsets),
                                                 n_records))

    def sync(self):
        _chk(self._L.pssbam_engine_sync(self._h))

    def reset(self):
        _chk(self._L.pssbam_engine_reset(self._h))

    def finish(self) -> Tables:
        fwd = rev = k5 = k3 = None
        if self.has_pss:
            fwd = np.zeros((self.region_len + 2, 16), dtype=np.uint64)
            rev = np.zeros_like(fwd)
        if self.has_kmer:
            k5 = np.zeros(4 ** self.klen, dtype=np.uint64)
            k3 = np.zeros_like(k5)
        st = np.zeros(ST_N, dtype=np.uint64)
        p = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        _chk(self._L.pssbam_engine_finish(self._h, p(fwd), p(rev), p(k5), p(k3), st.ctypes.data))
        return Tables(fwd, rev, k5, k3, {n: int(st[i]) for i, n in enumerate(ST_NAMES)})

    def counters_device(self) -> tuple[int, int]:
        ptr, n = C.c_void_p(), C.c_size_t()
        _chk(self._L.pssbam_engine_counters_device(self._h, C.byref(ptr), C.byref(n)))
        return int(ptr.value), int(n.value)

    def bind_counters(self, d_ptr: int | None, n_u64: int = 0):
        _chk(self._L.pssbam_engine_bind_counters(self._h, C.c_void_p(d_ptr) if d_ptr else None, n_u64))

    def counter_layout(self) -> dict:
        """u64-word offsets of the sections of the counter block"""
        rows = (self.region_len + 2) if self.has_pss else 0
        nb = 4 ** self.klen if self.has_kmer else 0
        lay = {"fwd": 0, "rev": rows * 16, "k5": 2 * rows * 16, "k3": 2 * rows * 16 + nb,
               "stats": 2 * rows * 16 + 2 * nb, "rows": rows, "bins": nb}
        # read groups: plane 0 (the unassigned bucket) is fwd / rev above; group g's [fwd | rev] pair follows the stats
        base = lay["stats"] + ST_N
        if not self.has_pss:   # k-mer planes: plane 0 is k5 / k3 above; plane k's [k5 | k3] pair follows the stats
            for name, tag, keys in (("groups", "id", self.read_groups), ("length_bins", "bin", self.length_bins),
                                    ("contig_sets", "label", self.contig_sets)):
                lay[name] = [{tag: key, "k5": base + k * 2 * nb, "k3": base + k * 2 * nb + nb} for k, key in enumerate(keys)]
            lay["n_u64"] = base + (len(self.read_groups) + len(self.length_bins) + len(self.contig_sets)) * 2 * nb
            return lay
        lay["groups"] = [{"id": g, "fwd": base + k * 2 * rows * 16, "rev": base + k * 2 * rows * 16 + rows * 16}
                         for k, g in enumerate(self.read_groups)]
        # length bins: bin k's pair sits where group k's would (plane 0 stays empty)
        lay["length_bins"] = [{"bin": b, "fwd": base + k * 2 * rows * 16, "rev": base + k * 2 * rows * 16 + rows * 16}
                              for k, b in enumerate(self.length_bins)]
        lay["contig_sets"] = [{"label": s, "fwd": base + k * 2 * rows * 16, "rev": base + k * 2 * rows * 16 + rows * 16}
                              for k, s in enumerate(self.contig_sets)]
        lay["n_u64"] = base + (len(self.read_groups) + len(self.length_bins) + len(self.contig_sets)) * 2 * rows * 16
        if self._replicates:   # read-name replicates (never together with the other planes): replicate j's pair sits where bin j's would
            lay["replicates"] = [{"replicate": j, "fwd": base + j * 2 * rows * 16, "rev": base + j * 2 * rows * 16 + rows * 16}
                                 for j in range(self._replicates)]
            lay["n_u64"] = base + self._replicates * 2 * rows * 16
        if self._per_contig:   # a plane per reference (never together with the other planes): plane k = refID k, k = n_ref: refID -1
            n_planes = 0 if self._n_ref is None else self._n_ref + 1   # (the block is sized once the count is known)
            lay["contigs"] = {"first": base, "plane_words": 2 * rows * 16, "n_planes": n_planes,
                              "touched": base + n_planes * 2 * rows * 16}
            lay["n_u64"] = base + n_planes * (2 * rows * 16 + 1)
        if self._length_hist:   # the length histogram (never together with planes): hf | hr behind the stats
            lay["hist_fwd"], lay["hist_rev"] = base, base + self._length_hist + 2
            lay["n_u64"] = base + 2 * (self._length_hist + 2)
        if self._site_context:   # site context (never together with planes or the histogram): fwd_in | rev_in behind the stats
            lay["site_fwd"], lay["site_rev"] = base, base + rows * 16
            lay["n_u64"] = base + 2 * rows * 16
        if self._end_condition[0]:   # the end condition (never together with any of the above): fwd_c | rev_c | reads[4]
            lay["end_fwd"], lay["end_rev"], lay["end_reads"] = base, base + rows * 16, base + 2 * rows * 16
            lay["n_u64"] = base + 2 * rows * 16 + 4
        if self._mismatches[0]:   # the mismatch histogram (never together with any of the above): mf | mr behind the stats
            lay["mism_fwd"], lay["mism_rev"] = base, base + self._mismatches[0] + 2
            lay["n_u64"] = base + 2 * (self._mismatches[0] + 2)
        if self._interior >= 0:   # the interior table (never together with any of the above): table[16] | reads behind the stats
            lay["interior"], lay["interior_reads"] = base, base + 16
            lay["n_u64"] = base + 17
        if self._composition:   # the composition table (never together with any of the above): c5 | c3 behind the stats
            lay["comp5"], lay["comp3"] = base, base + 10 * self._composition
            lay["n_u64"] = base + 20 * self._composition
        if self._read_score and self._read_score["hist_half"]:   # the score histogram (never together with any of the above): sf | sr
            lay["score_fwd"], lay["score_rev"] = base, base + 2 * self._read_score["hist_half"]
            lay["n_u64"] = base + 4 * self._read_score["hist_half"]
        return lay

    def genome_kmer_count(self, klen: int) -> np.ndarray:
        out = np.zeros(4 ** klen, dtype=np.uint64)
        _chk(self._L.pssbam_engine_genome_kmer_count(self._h, klen, out.ctypes.data))
        return out

    def timer_begin(self):
        _chk(self._L.pssbam_engine_timer_begin(self._h))

    def timer_end(self) -> float:
        ms = C.c_float()
        _chk(self._L.pssbam_engine_timer_end(self._h, C.byref(ms)))
        return float(ms.value)

    def kernel_time(self, reset: bool = True) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        _chk(self._L.pssbam_engine_kernel_time(self._h, C.byref(ms), C.byref(n), int(reset)))
        return float(ms.value), int(n.value)


class _Rescale(C.Structure):   # host/rescale.h pss_rescale
    _fields_ = [("mode", C.c_int), ("file_rows", C.c_uint32), ("rows", C.c_uint32), ("baseline", C.c_double * 2),
                ("rate", C.c_double * MAX_RESCALE_ROWS * 2), ("damage", C.c_double * MAX_RESCALE_ROWS * 2),
                ("table", C.c_uint8 * (2 * MAX_RESCALE_ROWS * RESCALE_QUALS))]


def rescale_table(path, mode: str, baseline: float | None = None) -> dict:
    """The quality-rescale table from the <prefix>.pss.rates.txt of an earlier run (pss_rescale_table, libpssbam_host.so): {"mode",
    "file_rows", "rows", "baseline" [2], "rate" [2][rows], "damage" [2][rows], "table" uint8 [2][rows][94]}, end 0 the 5' and 1 the
    3' end.  baseline None: the mean of each end's column over the second half of the file's rows.  PssbamError with the
    command's own message for a file it refuses."""
    H = C.CDLL(str(LIB_HOST))
    H.pss_rescale_table.argtypes = [C.c_char_p, C.c_int, C.c_double, C.POINTER(_Rescale), C.c_char_p, C.c_size_t]
    r, err = _Rescale(), C.create_string_buffer(700)
    if H.pss_rescale_table(str(path).encode(), RESCALE_MODES[mode], -1.0 if baseline is None else float(baseline), C.byref(r), err, len(err)):
        raise PssbamError(err.value.decode())
    n = int(r.rows)
    return {"mode": mode, "file_rows": int(r.file_rows), "rows": n, "baseline": [float(v) for v in r.baseline],
            "rate": np.array([list(r.rate[e])[:n] for e in range(2)]), "damage": np.array([list(r.damage[e])[:n] for e in range(2)]),
            "table": np.frombuffer(bytes(r.table), dtype=np.uint8)[:2 * n * RESCALE_QUALS].reshape(2, n, RESCALE_QUALS).copy()}

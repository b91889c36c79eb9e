"""pss-bam -w cost: what coverage_windows (csrc/coverage_kernels.h) takes per launch at human-genome size for three window sizes, beside
coverage_stats and a device-to-device copy of the array's bytes from the same session, what the call takes on the host, and what
writing the two text files takes.

    python tools/windows_bench.py [--reads 2000000] [--repeats 5] [--finish-positions 3100000000] [--windows 100,1000,1000000]
                                  [--out profiles/windows_bench.json]

The case is the finish case of tools/coverage_bench.py: one contig of --finish-positions bases and --reads 100-base reads spread over
its first 2^31 positions; the contig's letters repeat a block of 1 Mi random letters, nine in ten of them A C G T.  One profiled child
process per window size (`rocprofv3 --kernel-trace --stats`): 1 + --repeats rounds of {one record submitted, finish_coverage,
finish_coverage_windows}, so that each round computes anew; a kernel's ms per launch is its total duration over its calls.  The child of
the window size --text-window (default 1000) also times pss_write_windows of libpssbam_host.so into a temporary directory.  It measures
and records; it asserts only that the windows' depth sums add up to the contig's."""
import argparse
import csv
import ctypes as C
import json
import struct
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))

import coverage_bench as cb          # noqa: E402


def worker(a):
    pkg = cb.load_pkg(None)
    n, L, W = a.finish_positions, 100, a.worker
    name = b"r\0"
    one = struct.pack("<IiiBBHHHIiii", 32 + len(name) + 4 + L // 2 + L, 0, 0, len(name), 40, 0, 1, 0, L, -1, -1, 0) + name + struct.pack("<I", L << 4) + \
        bytes([0x11]) * (L // 2) + bytes([40]) * L
    recs = np.tile(np.frombuffer(one, dtype=np.uint8), a.reads).reshape(a.reads, len(one))
    pos = np.sort(np.random.default_rng(2).integers(2, min(n, 2 ** 31 - 1) - L - 2, size=a.reads)).astype("<i4")
    recs[:, 8:12] = pos.view(np.uint8).reshape(a.reads, 4)
    recs = recs.reshape(-1)
    offs = (np.arange(a.reads + 1, dtype=np.int64) * len(one)).astype(np.uint32)
    block = np.frombuffer(b"ACGTACGTNa", dtype=np.uint8)[np.random.default_rng(3).integers(0, 10, size=1 << 20)]
    genome = np.resize(block, n)
    eng = pkg.Engine(pss=dict(region_len=15, up_ctx="ACGTN", down_ctx="ACGTN"))
    eng.set_coverage(True, n)
    eng.set_genome_arrays([("big", genome)])
    eng.set_references(["big"])
    eng.submit(recs, offs)
    eng.sync()
    nbytes = 4 * cb.array_positions([n])
    copy_ms = cb.d2d_copy_ms(nbytes, 1 + a.repeats) if a.copy else []
    wall = {"finish_coverage_ms": [], "finish_coverage_windows_ms": []}
    one_rec, one_offs = recs[:len(one)].copy(), offs[:2].copy()
    n_win = eng.finish_coverage_windows(W, count_only=True)
    for _ in range(1 + a.repeats):
        eng.submit(one_rec, one_offs)                    # (something was added: the next finish computes anew)
        eng.sync()
        t0 = time.perf_counter()
        per, _, _ = eng.finish_coverage(1)
        t1 = time.perf_counter()
        win = eng.finish_coverage_windows(W, cap=n_win)
        t2 = time.perf_counter()
        wall["finish_coverage_ms"].append((t1 - t0) * 1e3)
        wall["finish_coverage_windows_ms"].append((t2 - t1) * 1e3)
    assert len(win[0]) == n_win and int(win[6].astype(object).sum()) == int(per[0, 1]) and int(win[5].astype(object).sum()) == int(per[0, 0])
    st = eng.finish().stats
    eng.close()
    row = {"window": W, "windows": n_win, "positions": n, "array_bytes": nbytes, "genome_bytes": n, "reads": a.reads, "pss_ok": st["pss_ok"], "calls": 1 + a.repeats,
           "depth_sum": int(per[0, 1]), "acgt": int(win[3].astype(object).sum()), "gc": int(win[4].astype(object).sum()),
           "host_wall": {k: v[1:] for k, v in wall.items()}}
    if a.copy:
        row.update({"d2d_copy_ms": copy_ms[1:], "d2d_copy_ms_best": min(copy_ms[1:])})
    if a.text:
        host = C.CDLL(str(pkg.LIB_HOST))
        u32p = C.POINTER(C.c_uint32)
        host.pss_write_windows.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_int, C.POINTER(C.c_char_p), C.c_uint64, C.POINTER(C.c_int32), u32p, u32p,
                                           u32p, u32p, u32p, C.POINTER(C.c_uint64)]
        names = (C.c_char_p * 1)(b"big")
        ptr = lambda v, t: v.ctypes.data_as(C.POINTER(t))  # noqa: E731
        with tempfile.TemporaryDirectory(prefix="windows_bench_") as td:
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                rc = host.pss_write_windows(b"f.fa", b"b.bam", str(Path(td) / "o").encode(), W, 1, names, n_win, ptr(win[0], C.c_int32),
                                            *[ptr(v, C.c_uint32) for v in win[1:6]], ptr(win[6], C.c_uint64))
                times.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            row["write_text_ms"] = times
            row["windows_txt_bytes"] = (Path(td) / "o.pss.windows.txt").stat().st_size
    print("WINDOWS_BENCH " + json.dumps(row))


def profiled(a, W: int, tmp: Path, first: bool):
    d = tmp / f"w{W}"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--", sys.executable, __file__, "--worker", str(W), "--reads", str(a.reads),
           "--repeats", str(a.repeats), "--finish-positions", str(a.finish_positions)] + (["--copy"] if first else []) + (["--text"] if W == a.text_window else [])
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("WINDOWS_BENCH ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(f"{' '.join(cmd)}\n{pr.stdout[-2000:]}\n{pr.stderr[-2000:]}")
    row = json.loads(line[0][len("WINDOWS_BENCH "):])
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            for key, kernel in (("windows_ms", "coverage_windows"), ("stats_ms", "coverage_stats"), ("tile_sums_ms", "coverage_tile_sums")):
                if kernel in r["Name"]:
                    row[key] = float(r["TotalDurationNs"]) / max(int(r["Calls"]), 1) / 1e6     # per launch of the kernel
                    row[key.replace("_ms", "_calls")] = int(r["Calls"])
    row["windows_over_stats"] = row["windows_ms"] / row["stats_ms"]
    row["read_bytes_per_launch"] = row["array_bytes"] + row["genome_bytes"]
    row["windows_read_gb_per_s"] = row["read_bytes_per_launch"] / row["windows_ms"] / 1e6
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--finish-positions", type=int, default=3_100_000_000)
    ap.add_argument("--windows", default="100,1000,1000000")
    ap.add_argument("--text-window", type=int, default=1000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "windows_bench.json"))
    ap.add_argument("--worker", type=int, default=None)   # (the profiled child: its window size)
    ap.add_argument("--copy", action="store_true")
    ap.add_argument("--text", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rows = []
    with tempfile.TemporaryDirectory(prefix="windows_bench_") as td:
        for k, W in enumerate(int(w) for w in a.windows.split(",")):
            rows.append(profiled(a, W, Path(td), k == 0))
            print(json.dumps(rows[-1]), flush=True)
    copy = rows[0]["d2d_copy_ms_best"]
    for r in rows:
        r["windows_over_copy"] = r["windows_ms"] / copy
        r["stats_over_copy"] = r["stats_ms"] / copy
    sec = {"statistic": "one profiled process per window size: kernel ms per launch = rocprofv3 --kernel-trace --stats total duration of the kernel over its calls, 1 + "
                        "repeats rounds of {one record submitted, finish_coverage, finish_coverage_windows}; coverage_windows reads 5 bytes per position (4 of the "
                        "array, 1 of the genome), coverage_stats 4; d2d copy: hipMemcpyAsync of the array's bytes between two events, best of repeats, first process; "
                        "host_wall: time.perf_counter around the wrapper's call, first round left out; write_text_ms: pss_write_windows of both files, three times",
           "repeats": a.repeats, "reads": a.reads, "rows": rows}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    main()

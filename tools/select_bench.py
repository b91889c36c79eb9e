"""pss-bam -O cost: what the record sink's three device steps (mark, scan, gather: csrc/select_kernels.h) take per launch beside the
tally launch they follow, what a plain device-to-device copy of the kept bytes takes (the gather's ceiling), and what the whole
command takes with and without -O.

    python tools/select_bench.py [--reads 4000000] [--repeats 5] [--scale-genome 0.02] [--parent-lib <libpssbam_hip.so of the
                                 commit before the sink>] [--cli-reads 4000000] [--out profiles/select_bench.json]

Workloads: the synthetic C1 (100-base reads, one contig) and C4 (30..80-base reads, CIGAR mix, duplicates, low MAPQ) records
of bench.py's generator, one block of --reads records; kept fractions of about 5 %, 50 % and 100 %, set with -T intervals that
cover that share of every contig (the figure kept is recorded).  Kernel times come from `rocprofv3 --kernel-trace --stats`, one
profiled child process per (workload, fraction): the average duration per call of select_mark, of the three scan kernels
together, of select_gather and of the tally launch (tally kernel + its reduce) over --repeats submits behind one warm-up.  With
--parent-lib the same child is run once more on that library without a sink: the tally launch at the parent commit.  The copy
is timed with HIP events in a child of its own, the profiler off (best of --repeats, warmed).  The command's wall time is taken
--cli-runs times each way, alternating, behind one warm-up pair, on a BAM and FASTA written from C4 with `-L 32` (about 5 % kept),
the profiler off; the file gives every run, the smallest, the median and the largest, and whether the two ranges overlap.
It measures and records; it asserts only that the sink delivered what pss_ok counted."""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
FRACTIONS = (0.05, 0.5, 1.0)
SCAN_KERNELS = ("select_tile_sums", "select_scan_sums", "select_scan_tiles")


def load_pkg(lib: str | None):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    if lib:
        pkg.LIB_HIP = Path(lib)
    return pkg


def workload(pkg, name: str, reads: int, scale: float):
    from pss_bam_amd import synth
    d = synth.config(name, n_reads=reads, scale_genome=scale)
    region_len = d.pop("region_len")
    d.pop("klen", None)
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, reads, threads=16)
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(int(scfg.n_contigs))]
    return scfg, recs, offs, names, genome, region_len


def worker(a):
    """one engine, one block, warm-up + repeats submits; prints one JSON line"""
    pkg = load_pkg(a.lib)
    scfg, recs, offs, names, genome, region_len = workload(pkg, a.worker, a.reads, a.scale_genome)
    eng = pkg.Engine(pss=dict(region_len=region_len))
    if a.fraction < 1.0:
        eng.set_regions(names, np.arange(len(names), dtype=np.int32), np.zeros(len(names), dtype=np.uint32),
                        np.array([max(1, int(g.size * a.fraction)) for _, g in genome], dtype=np.uint32))
    got = {"bytes": 0, "records": 0}

    def sink(chunk, n):
        got["bytes"] += chunk.size
        got["records"] += n

    if not a.no_sink:
        eng.set_record_sink(sink)
    eng.set_genome_arrays(genome)
    eng.set_references(names)
    for _ in range(1 + a.repeats):
        eng.submit(recs, offs)
        eng.sync()
    ms, launches = eng.kernel_time()
    st = eng.finish().stats
    eng.close()
    n_sub = 1 + a.repeats
    out = {"workload": a.worker, "fraction_asked": a.fraction, "reads": a.reads, "block_bytes": int(offs[-1]), "region_len": region_len,
           "pss_ok": st["pss_ok"] // n_sub, "kept_records": got["records"] // n_sub, "kept_bytes": got["bytes"] // n_sub,
           "tally_ms_by_events": ms / n_sub, "tally_launches_per_submit": launches / n_sub}
    if not a.no_sink:
        assert got["records"] == st["pss_ok"], (got, st)
        out["fraction_kept"] = out["kept_records"] / a.reads
    print("SELECT_BENCH " + json.dumps(out))


def d2d_copy_ms(nbytes: int, repeats: int) -> float:
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    src, dst, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), nbytes) == 0 and hip.hipMalloc(C.byref(dst), nbytes) == 0
    assert hip.hipMemset(src, 1, nbytes) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    best = None
    for k in range(1 + repeats):
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(dst, src, nbytes, 3, None) == 0          # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        if k:
            best = ms.value if best is None else min(best, ms.value)
    hip.hipFree(src)
    hip.hipFree(dst)
    return best


def copy_unprofiled(a, nbytes: int) -> float:
    """the device-to-device copy, in a process of its own without the profiler"""
    pr = subprocess.run([sys.executable, __file__, "--copy-only", str(nbytes), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=300)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("SELECT_COPY ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(pr.stdout[-1000:] + pr.stderr[-1000:])
    return float(line[0].split()[1])


def profiled(a, name: str, fraction: float, lib: str | None, no_sink: bool, tmp: Path) -> dict:
    d = tmp / f"{name}_{fraction}_{'parent' if lib else 'now'}"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--", sys.executable, __file__,
           "--worker", name, "--fraction", str(fraction), "--reads", str(a.reads), "--repeats", str(a.repeats),
           "--scale-genome", str(a.scale_genome)] + (["--lib", lib] if lib else []) + (["--no-sink"] if no_sink else [])
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("SELECT_BENCH ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(f"{' '.join(cmd)}\n{pr.stdout[-2000:]}\n{pr.stderr[-2000:]}")
    row = json.loads(line[0][len("SELECT_BENCH "):])
    per_call = {}
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            per_call[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    n_sub = 1 + a.repeats

    def ms_per_submit(pred):
        return sum(t for k, (c, t) in per_call.items() if pred(k)) / n_sub / 1e6

    row["tally_ms"] = ms_per_submit(lambda k: "pssbam::tally_" in k or "pssbam::reduce_partials" in k)
    if not no_sink:
        row["mark_ms"] = ms_per_submit(lambda k: "select_mark" in k)
        row["scan_ms"] = ms_per_submit(lambda k: any(s in k for s in SCAN_KERNELS))
        row["gather_ms"] = ms_per_submit(lambda k: "select_gather" in k)
        row["select_launches_per_submit"] = sum(c for k, (c, _) in per_call.items() if "pssbam::select_" in k) / n_sub
    return row


def cli_wall(a, pkg, tmp: Path) -> dict:
    from pss_bam_amd import synth
    d = synth.config("C4", n_reads=a.cli_reads, scale_genome=a.scale_genome)
    d.pop("region_len")
    scfg = synth.make_cfg(**d)
    fa, bam = tmp / "ref.fa", tmp / "reads.bam"
    synth.fasta_host(scfg, fa, threads=16)
    synth.bam_file_host(scfg, 0, a.cli_reads, bam, level=1, threads=16)
    exe = str(pkg.PKG_DIR / "bin" / "pss-bam")
    base = [exe, "-F", str(fa), "-B", str(bam), "-L", "32"]
    times = {"without_O": [], "with_O": []}
    kept = None
    for k in range(1 + a.cli_runs):                      # (the first pair warms the page cache and is left out)
        for key, more in (("without_O", ["-o", str(tmp / "p")]), ("with_O", ["-o", str(tmp / "o"), "-O", str(tmp / "kept.bam")])):
            t0 = time.perf_counter()
            pr = subprocess.run(base + more, capture_output=True, text=True, env={**os.environ, "PSSBAM_STATS": "1"}, timeout=900)
            dt = time.perf_counter() - t0
            if pr.returncode != 0:
                raise RuntimeError(pr.stderr[-2000:])
            if k:
                times[key].append(dt)
            kept = int([ln for ln in pr.stderr.splitlines() if ln.startswith("[pssbam] pss_ok=")][0].split("=")[1])
    assert (tmp / "p.pss.counts.txt").read_text().split("\n", 4)[4] == (tmp / "o.pss.counts.txt").read_text().split("\n", 4)[4]
    return {"reads": a.cli_reads, "options": "-L 32", "bam_bytes": bam.stat().st_size, "kept_records": kept, "fraction_kept": kept / a.cli_reads,
            "kept_bam_bytes": (tmp / "kept.bam").stat().st_size, "wall_s": times,
            "min_wall_s": {k: min(v) for k, v in times.items()}, "median_wall_s": {k: statistics.median(v) for k, v in times.items()},
            "max_wall_s": {k: max(v) for k, v in times.items()},
            "ranges_overlap": max(times["without_O"]) >= min(times["with_O"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--cli-reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cli-runs", type=int, default=7)
    ap.add_argument("--copy-only", type=int, default=0)  # (the unprofiled copy child)
    ap.add_argument("--scale-genome", type=float, default=0.02)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "select_bench.json"))
    ap.add_argument("--worker", default=None)            # (the profiled child)
    ap.add_argument("--fraction", type=float, default=1.0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--no-sink", action="store_true")
    a = ap.parse_args()
    if a.copy_only:
        print(f"SELECT_COPY {d2d_copy_ms(a.copy_only, a.repeats)}")
        return
    if a.worker:
        return worker(a)
    pkg = load_pkg(None)
    rows = []
    with tempfile.TemporaryDirectory(prefix="select_bench_") as td:
        tmp = Path(td)
        for name in ("C1", "C4"):
            for frac in FRACTIONS:
                row = profiled(a, name, frac, None, False, tmp)
                if a.parent_lib:
                    par = profiled(a, name, frac, a.parent_lib, True, tmp)
                    assert par["pss_ok"] == row["pss_ok"], (par, row)
                    row["parent_tally_ms"] = par["tally_ms"]
                row["d2d_copy_ms"] = copy_unprofiled(a, max(row["kept_bytes"], 1))
                sel = row["mark_ms"] + row["scan_ms"] + row["gather_ms"]
                row["select_over_tally"] = sel / row["tally_ms"]
                row["mark_over_tally"] = row["mark_ms"] / row["tally_ms"]
                row["gather_over_d2d_copy"] = row["gather_ms"] / row["d2d_copy_ms"]
                rows.append(row)
                print(json.dumps(row), flush=True)
        cli = cli_wall(a, pkg, tmp)
    sec = {"statistic": "kernel ms per submit: rocprofv3 --kernel-trace --stats totals over 1 warm-up + repeats submits of one block, divided by the "
                        "submits; d2d_copy_ms: hipMemcpyAsync device to device of kept_bytes, HIP events, best of repeats, in an unprofiled process; wall_s: the whole command, "
                        "cli_runs runs each way behind one warm-up pair, alternating, profiler off",
           "cli_runs": a.cli_runs,
           "repeats": a.repeats, "scale_genome": a.scale_genome, "blocks": rows, "command": cli}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    main()

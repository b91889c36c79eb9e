"""pss-bam -O ... -Z cost: what the block sink's device steps (bgzf_deflate, bgzf_pack_scan, bgzf_pack_copy: csrc/deflate_kernels.h)
take per submit, how large their output is beside what bam_writer's zlib level 1 makes of the same bytes, and what the whole
command takes with -O ... -Z against -O ... -z 1 of the same build.

    python tools/deflate_bench.py [--reads 2000000] [--repeats 3] [--scale-genome 0.02] [--cli-reads 2000000] [--cli-runs 7]
                                  [--out profiles/deflate_bench.json]

Workloads: the synthetic C1 and C4 records of bench.py's generator, one block of --reads records, at the kept fractions of
tools/select_bench.py (-T intervals over about 5 %, 50 % and 100 % of every contig; the figure kept is recorded).  Kernel times
come from `rocprofv3 --kernel-trace --stats`, one profiled child process per (workload, fraction), in runs of their own: the
duration per submit of bgzf_deflate and of the two pack kernels over --repeats submits behind one warm-up, beside the select
kernels and the tally launch of the same submits.  The size: the bytes the sink received, beside the sum over the same payloads
(the kept stream cut every 0xFF00 bytes) of zlib level 1's raw deflate + 26 bytes of frame -- what bam_writer writes per block
at -z 1, up to where it cuts.  The command's wall time is taken --cli-runs times each way, alternating, behind one warm-up
pair, the profiler off, on a BAM and FASTA written from C4 with no filter option (the unfiltered kept fraction); the file gives
every run, the smallest, the median and the largest, and whether the two ranges overlap.  It measures and records; it asserts
only that the blocks inflate to as many bytes as the sink was told and hold what pss_ok counted."""
import argparse
import csv
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
FRACTIONS = (0.05, 0.5, 1.0)
PAYLOAD = 0xFF00

sys.path.insert(0, str(ROOT / "tools"))
from select_bench import load_pkg, workload  # noqa: E402


def worker(a):
    """one engine with a block sink, one block, warm-up + repeats submits; prints one JSON line"""
    pkg = load_pkg(None)
    scfg, recs, offs, names, genome, region_len = workload(pkg, a.worker, a.reads, a.scale_genome)
    eng = pkg.Engine(pss=dict(region_len=region_len))
    if a.fraction < 1.0:
        eng.set_regions(names, np.arange(len(names), dtype=np.int32), np.zeros(len(names), dtype=np.uint32),
                        np.array([max(1, int(g.size * a.fraction)) for _, g in genome], dtype=np.uint32))
    got = {"bytes": 0, "blocks": 0, "raw": 0, "records": 0}
    last = []

    def sink(chunk, n_blocks, raw_bytes, n):
        got["bytes"] += chunk.size
        got["blocks"] += n_blocks
        got["raw"] += raw_bytes
        got["records"] += n
        last[:] = [chunk]

    eng.set_block_sink(sink)
    eng.set_genome_arrays(genome)
    eng.set_references(names)
    for _ in range(1 + a.repeats):
        eng.submit(recs, offs)
        eng.sync()
    st = eng.finish().stats
    eng.close()
    n_sub = 1 + a.repeats
    assert got["records"] == st["pss_ok"], (got, st)
    out = {"workload": a.worker, "fraction_asked": a.fraction, "reads": a.reads, "block_bytes": int(offs[-1]),
           "kept_records": got["records"] // n_sub, "fraction_kept": got["records"] / n_sub / a.reads, "kept_bytes": got["raw"] // n_sub,
           "bgzf_blocks": got["blocks"] // n_sub, "bgzf_bytes": got["bytes"] // n_sub}
    # the same payloads through zlib level 1, after the kernels were timed (the last chunk, inflated with the host's zlib)
    raw = gzip.decompress(last[0].tobytes()) if last else b""
    assert len(raw) == out["kept_bytes"]
    z1 = 0
    for o in range(0, len(raw), PAYLOAD):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        z1 += 26 + len(c.compress(raw[o:o + PAYLOAD]) + c.flush())
    out["zlib1_bytes"] = z1
    print("DEFLATE_BENCH " + json.dumps(out))


def profiled(a, name: str, fraction: float, tmp: Path) -> dict:
    d = tmp / f"{name}_{fraction}"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--", sys.executable, __file__,
           "--worker", name, "--fraction", str(fraction), "--reads", str(a.reads), "--repeats", str(a.repeats),
           "--scale-genome", str(a.scale_genome)]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("DEFLATE_BENCH ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(f"{' '.join(cmd)}\n{pr.stdout[-2000:]}\n{pr.stderr[-2000:]}")
    row = json.loads(line[0][len("DEFLATE_BENCH "):])
    per_call = {}
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            per_call[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    n_sub = 1 + a.repeats

    def ms_per_submit(pred):
        return sum(t for k, (c, t) in per_call.items() if pred(k)) / n_sub / 1e6

    row["tally_ms"] = ms_per_submit(lambda k: "pssbam::tally_" in k or "pssbam::reduce_partials" in k)
    row["select_ms"] = ms_per_submit(lambda k: "pssbam::select_" in k)
    row["deflate_ms"] = ms_per_submit(lambda k: "bgzf_deflate" in k)
    row["pack_ms"] = ms_per_submit(lambda k: "bgzf_pack_" in k)
    row["deflate_launches_per_submit"] = sum(c for k, (c, _) in per_call.items() if "bgzf_deflate" in k or "bgzf_pack_" in k) / n_sub
    row["deflate_GBps_of_kept_bytes"] = row["kept_bytes"] / 1e6 / row["deflate_ms"] if row["deflate_ms"] else None
    row["size_over_zlib1"] = row["bgzf_bytes"] / row["zlib1_bytes"] if row["zlib1_bytes"] else None
    row["size_over_raw"] = row["bgzf_bytes"] / row["kept_bytes"] if row["kept_bytes"] else None
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
    base = [exe, "-F", str(fa), "-B", str(bam)]
    ways = (("O_z1", ["-o", str(tmp / "z"), "-O", str(tmp / "z1.bam"), "-z", "1"]), ("O_Z", ["-o", str(tmp / "g"), "-O", str(tmp / "gpu.bam"), "-Z"]))
    times = {k: [] for k, _ in ways}
    kept = None
    for k in range(1 + a.cli_runs):                      # (the first pair warms the page cache and is left out)
        for key, more in ways:
            t0 = time.perf_counter()
            pr = subprocess.run(base + more, capture_output=True, text=True, env={**os.environ, "PSSBAM_STATS": "1"}, timeout=900)
            dt = time.perf_counter() - t0
            if pr.returncode != 0:
                raise RuntimeError(pr.stderr[-2000:])
            if k:
                times[key].append(dt)
            kept = int([ln for ln in pr.stderr.splitlines() if ln.startswith("[pssbam] pss_ok=")][0].split("=")[1])
    same = subprocess.run(["cmp", str(tmp / "z.pss.counts.txt"), str(tmp / "g.pss.counts.txt")], capture_output=True).returncode
    return {"reads": a.cli_reads, "options": "none (the unfiltered kept fraction)", "bam_bytes": bam.stat().st_size, "kept_records": kept,
            "fraction_kept": kept / a.cli_reads, "kept_bam_bytes": {"O_z1": (tmp / "z1.bam").stat().st_size, "O_Z": (tmp / "gpu.bam").stat().st_size},
            "tables_differ_only_in_their_header_lines": same in (0, 1), "wall_s": times,
            "min_wall_s": {k: min(v) for k, v in times.items()}, "median_wall_s": {k: statistics.median(v) for k, v in times.items()},
            "max_wall_s": {k: max(v) for k, v in times.items()},
            "ranges_overlap": max(times["O_Z"]) >= min(times["O_z1"]) and max(times["O_z1"]) >= min(times["O_Z"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--cli-reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cli-runs", type=int, default=7)
    ap.add_argument("--scale-genome", type=float, default=0.02)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "deflate_bench.json"))
    ap.add_argument("--worker", default=None)            # (the profiled child)
    ap.add_argument("--fraction", type=float, default=1.0)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    pkg = load_pkg(None)
    rows = []
    with tempfile.TemporaryDirectory(prefix="deflate_bench_") as td:
        tmp = Path(td)
        for name in ("C1", "C4"):
            for frac in FRACTIONS:
                row = profiled(a, name, frac, tmp)
                rows.append(row)
                print(json.dumps(row), flush=True)
        cli = None if a.skip_cli else cli_wall(a, pkg, tmp)
    sec = {"statistic": "kernel ms per submit: rocprofv3 --kernel-trace --stats totals over 1 warm-up + repeats submits of one block, divided by the "
                        "submits; zlib1_bytes: zlib level 1 raw deflate + 26 bytes of frame over the same 0xFF00-byte payloads; wall_s: the whole command, "
                        "cli_runs runs each way behind one warm-up pair, alternating, profiler off",
           "cli_runs": a.cli_runs, "repeats": a.repeats, "scale_genome": a.scale_genome, "blocks": rows, "command": cli}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    main()

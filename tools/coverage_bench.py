"""pss-bam -c / -b cost: what coverage_add (csrc/coverage_kernels.h) takes per submit beside the tally launch it follows, what the
finish kernels take at human-genome size beside a device-to-device copy of the array's bytes, and whether the tally launch with the
setting off still takes what it took at the parent commit.

    python tools/coverage_bench.py [--reads 2000000] [--repeats 5] [--runs 3] [--scale-genome 0.02] [--finish-positions 3100000000]
                                   [--parent-lib <libpssbam_hip.so of the commit before the setting>] [--out profiles/coverage_bench.json]

Blocks: the synthetic C1 (100-base reads, one contig) and C4 (30..80-base reads, CIGAR mix, duplicates, low MAPQ) records of bench.py's
generator, one block of --reads records, sorted by (refID, POS) and shuffled.  Kernel times come from `rocprofv3 --kernel-trace --stats`,
one profiled child process per row: the total duration of each kernel family over 1 warm-up + --repeats submits of the block (a reset
in front of each), divided by the submits.  Finish: one contig of --finish-positions bases, all A, and --reads 100-base reads of A
spread over its first 2^31 positions (BAM's POS is 32 bits signed); a submit of one record in front of each
finish_coverage, so that it computes anew, and finish_coverage_runs behind it, 1 + --repeats times; the copy is hipMemcpyAsync
device-to-device of the array's bytes (zeroed) between two events, best of --repeats.  With --parent-lib
the setting-off tally launch is taken --runs times on each library, alternating; the file gives every run and whether the two ranges
overlap.  It measures and records; it asserts only that both libraries tallied the same reads."""
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
FINISH = {"tile_sums_ms": "coverage_tile_sums", "scan_sums_ms": "coverage_scan_sums", "stats_ms": "coverage_stats", "runs_ms": "coverage_runs"}


def load_pkg(lib: str | None):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    if lib:
        pkg.LIB_HIP = Path(lib)
    return pkg


def workload(name: str, reads: int, scale: float, order: str):
    from pss_bam_amd import synth
    d = synth.config(name, n_reads=reads, scale_genome=scale)
    region_len = d.pop("region_len")
    d.pop("klen", None)
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, reads, threads=16)
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(int(scfg.n_contigs))]
    offs64 = offs.astype(np.int64)
    field = lambda at: (recs[offs64[:-1, None] + at + np.arange(4)].astype(np.uint32) << (8 * np.arange(4, dtype=np.uint32))).sum(axis=1)  # noqa: E731
    idx = np.lexsort((field(8), field(4))) if order == "sorted" else np.random.default_rng(1).permutation(reads)
    lens = (offs64[1:] - offs64[:-1])[idx]
    new_offs = np.concatenate([[0], np.cumsum(lens)])
    src = np.repeat(offs64[idx] - new_offs[:-1], lens) + np.arange(new_offs[-1])
    return np.ascontiguousarray(recs[src]), new_offs.astype(np.uint32), names, genome, region_len


def block_worker(a):
    """one engine, one block, warm-up + repeats submits behind a reset each; prints one JSON line"""
    pkg = load_pkg(a.lib)
    recs, offs, names, genome, region_len = workload(a.worker, a.reads, a.scale_genome, a.order)
    eng = pkg.Engine(pss=dict(region_len=region_len))
    if a.mode == "on":
        eng.set_coverage(True)
    eng.set_genome_arrays(genome)
    eng.set_references(names)
    n_sub = 1 + a.repeats
    for _ in range(n_sub):
        eng.reset()
        eng.submit(recs, offs)
        eng.sync()
    ms, launches = eng.kernel_time()
    cov = None
    if a.mode == "on":
        per, hist, n_runs = eng.finish_coverage(len(names))
        cov = {"covered": int(per[:, 0].sum()), "depth_sum": int(per[:, 1].sum()), "max_depth": int(per[:, 2].max()), "runs": n_runs}
    st = eng.finish().stats
    eng.close()
    print("COVERAGE_BENCH " + json.dumps({"workload": a.worker, "order": a.order, "mode": a.mode, "reads": int(offs.size - 1), "block_bytes": int(offs[-1]),
                                          "region_len": region_len, "submits": n_sub, "pss_ok": st["pss_ok"], "tally_launches_per_submit": launches / n_sub,
                                          "coverage": cov}))


def array_positions(contig_lens) -> int:
    """the engine's array for a genome of these contigs: 256 positions in front, every contig with 256 of padding rounded up to 256
    (csrc/engine.hip: CONTIG_PAD, CONTIG_ALIGN), the whole rounded up to tiles of 4096 (csrc/coverage_kernels.h: COV_TILE)"""
    total = 256 + sum((ln + 256 + 255) // 256 * 256 for ln in contig_lens)
    return (total + 4095) // 4096 * 4096


def d2d_copy_ms(nbytes: int, times: int) -> list:
    """hipMemcpyAsync device to device of nbytes zeroed bytes on the null stream, between two events; two buffers of that size beside
    whatever the engine holds"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    src, dst, e0, e1, out = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), []
    assert hip.hipMalloc(C.byref(src), nbytes) == 0 and hip.hipMalloc(C.byref(dst), nbytes) == 0
    assert hip.hipMemset(src, 0, nbytes) == 0 and hip.hipMemset(dst, 0, nbytes) == 0
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    for _ in range(times):
        assert hip.hipEventRecord(e0, None) == 0 and hip.hipMemcpyAsync(dst, src, nbytes, 3, None) == 0 and hip.hipEventRecord(e1, None) == 0
        assert hip.hipEventSynchronize(e1) == 0
        ms = C.c_float(0)
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        out.append(float(ms.value))
    for ev in (e0, e1):
        hip.hipEventDestroy(ev)
    hip.hipFree(src)
    hip.hipFree(dst)
    return out


def finish_worker(a):
    pkg = load_pkg(a.lib)
    n, L = a.finish_positions, 100
    name = b"r\0"
    one = struct.pack("<IiiBBHHHIiii", 32 + len(name) + 4 + L // 2 + L, 0, 0, len(name), 40, 0, 1, 0, L, -1, -1, 0) + name + struct.pack("<I", L << 4) + \
        bytes([0x11]) * (L // 2) + bytes([40]) * L
    recs = np.tile(np.frombuffer(one, dtype=np.uint8), a.reads).reshape(a.reads, len(one))
    pos = np.sort(np.random.default_rng(2).integers(2, min(n, 2 ** 31 - 1) - L - 2, size=a.reads)).astype("<i4")
    recs[:, 8:12] = pos.view(np.uint8).reshape(a.reads, 4)
    recs = recs.reshape(-1)
    offs = (np.arange(a.reads + 1, dtype=np.int64) * len(one)).astype(np.uint32)
    eng = pkg.Engine(pss=dict(region_len=15))
    eng.set_coverage(True, n)
    eng.set_genome_arrays([("big", np.full(n, ord("A"), dtype=np.uint8))])
    eng.set_references(["big"])
    eng.submit(recs, offs)
    eng.sync()
    nbytes = 4 * array_positions([n])
    copy_ms = d2d_copy_ms(nbytes, 1 + a.repeats)
    wall = {"finish_coverage_ms": [], "finish_coverage_runs_ms": []}
    one_rec, one_offs = recs[:len(one)].copy(), offs[:2].copy()
    for _ in range(1 + a.repeats):
        eng.submit(one_rec, one_offs)                    # (something was added: the next finish computes anew)
        eng.sync()
        t0 = time.perf_counter()
        per, hist, n_runs = eng.finish_coverage(1)
        t1 = time.perf_counter()
        runs = eng.finish_coverage_runs(cap=n_runs)
        t2 = time.perf_counter()
        wall["finish_coverage_ms"].append((t1 - t0) * 1e3)
        wall["finish_coverage_runs_ms"].append((t2 - t1) * 1e3)
    st = eng.finish().stats
    eng.close()
    print("COVERAGE_BENCH " + json.dumps({"positions": n, "array_bytes": nbytes, "reads": a.reads, "pss_ok": st["pss_ok"], "runs": n_runs, "calls": 1 + a.repeats,
                                          "covered": int(per[0, 0]), "max_depth": int(per[0, 2]), "d2d_copy_ms": copy_ms[1:], "d2d_copy_ms_best": min(copy_ms[1:]),
                                          "host_wall": {k: v[1:] for k, v in wall.items()}, "runs_returned": int(len(runs[0]))}))


def profiled(a, args: list, lib: str | None, tmp: Path, tag: str):
    d = tmp / tag
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--", sys.executable, __file__, *args, "--reads", str(a.reads),
           "--repeats", str(a.repeats), "--scale-genome", str(a.scale_genome), "--finish-positions", str(a.finish_positions)] + (["--lib", lib] if lib else [])
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("COVERAGE_BENCH ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(f"{' '.join(cmd)}\n{pr.stdout[-2000:]}\n{pr.stderr[-2000:]}")
    row = json.loads(line[0][len("COVERAGE_BENCH "):])
    per_call = {}
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            per_call[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    return row, (lambda pred: [(c, t) for k, (c, t) in per_call.items() if pred(k)])


def block_row(a, name, order, mode, lib, tmp, tag):
    row, pick = profiled(a, ["--worker", name, "--order", order, "--mode", mode], lib, tmp, f"{name}_{order}_{mode}_{tag}")
    row["tally_ms"] = sum(t for _, t in pick(lambda k: "pssbam::tally_" in k or "pssbam::reduce_partials" in k)) / row["submits"] / 1e6
    if mode == "on":
        row["coverage_add_ms"] = sum(t for _, t in pick(lambda k: "coverage_add" in k)) / row["submits"] / 1e6
        row["coverage_add_over_tally"] = row["coverage_add_ms"] / row["tally_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=0.02)
    ap.add_argument("--finish-positions", type=int, default=3_100_000_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "coverage_bench.json"))
    ap.add_argument("--worker", default=None)            # (the profiled child: a workload's name, or "finish")
    ap.add_argument("--order", default="sorted", choices=["sorted", "shuffled"])
    ap.add_argument("--mode", default="on", choices=["on", "off"])
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.worker == "finish":
        return finish_worker(a)
    if a.worker:
        return block_worker(a)
    rows, off = [], []
    with tempfile.TemporaryDirectory(prefix="coverage_bench_") as td:
        tmp = Path(td)
        for name in ("C1", "C4"):
            for order in ("sorted", "shuffled"):
                row = block_row(a, name, order, "on", None, tmp, "now")
                rows.append(row)
                print(json.dumps(row), flush=True)
        fin, pick = profiled(a, ["--worker", "finish"], None, tmp, "finish")
        for key, kernel in FINISH.items():
            calls = sum(c for c, _ in pick(lambda k: kernel in k))
            fin[key] = sum(t for _, t in pick(lambda k: kernel in k)) / max(calls, 1) / 1e6      # per launch of the kernel
            fin[key.replace("_ms", "_calls")] = calls
        fin["summary_kernels_ms"] = fin["tile_sums_ms"] + fin["scan_sums_ms"] + fin["stats_ms"]
        fin["summary_kernels_over_copy"] = fin["summary_kernels_ms"] / fin["d2d_copy_ms_best"]
        print(json.dumps(fin), flush=True)
        for name in ("C1", "C4"):
            runs = {"now": [], "parent": []}
            for k in range(a.runs):                      # alternating, so that drift of the machine shows in both
                for key, lib in (("now", None), ("parent", a.parent_lib)):
                    if key == "parent" and not lib:
                        continue
                    runs[key].append(block_row(a, name, "sorted", "off", lib, tmp, f"{key}{k}"))
            assert len({r["pss_ok"] for rr in runs.values() for r in rr}) == 1, runs
            ms = {k: [r["tally_ms"] for r in v] for k, v in runs.items() if v}
            entry = {"workload": name, "reads": a.reads, "tally_ms_setting_off": ms, "min": {k: min(v) for k, v in ms.items()},
                     "max": {k: max(v) for k, v in ms.items()}, "tally_launches_per_submit": runs["now"][0]["tally_launches_per_submit"]}
            if "parent" in ms:
                entry["ranges_overlap"] = max(ms["now"]) >= min(ms["parent"]) and max(ms["parent"]) >= min(ms["now"])
            off.append(entry)
            print(json.dumps(entry), flush=True)
    sec = {"statistic": "blocks: kernel ms per submit, rocprofv3 --kernel-trace --stats totals of a kernel family over 1 warm-up + repeats submits of one block "
                        "(a reset in front of each), divided by the submits; tally = the tally kernel + its reduce; finish: ms per launch of each kernel over 1 + "
                        "repeats pairs of finish_coverage (tile_sums, scan_sums, stats; one record submitted in front of it) and finish_coverage_runs (scan_sums "
                        "over the run counts, runs); summary_kernels_ms = tile_sums + scan_sums + stats, one finish_coverage; d2d copy: hipMemcpyAsync of the "
                        "array's bytes between two events; setting off: the tally launch of "
                        "`runs` processes per library, alternating",
           "repeats": a.repeats, "runs": a.runs, "scale_genome": a.scale_genome, "blocks": rows, "finish": fin, "setting_off": off}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    main()

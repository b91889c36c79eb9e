"""pss-bam -K cost: what the end mask's one kernel (select_mask_ends, csrc/end_mask_kernels.h) takes per launch beside the
select_gather it follows and beside the tally launch of the same block; and whether the path without a mask moved: select_gather
and the tally on this build and on the build of the commit before the mask, in turn.

    python tools/end_mask_bench.py [--reads 2000000] [--repeats 5] [--rounds 2] [--scale-genome 0.02]
                                   [--parent-lib <libpssbam_hip.so of the commit before the mask>] [--out profiles/end_mask_bench.json]

Workloads, blocks and kept fractions are those of tools/select_bench.py: the synthetic C1 (100-base reads, one contig) and C4
(30..80-base reads, CIGAR mix, duplicates, low MAPQ) records of bench.py's generator, one block of --reads records; about 5 %,
50 % and 100 % kept, set with -T intervals that cover that share of every contig.  Kernel times come from `rocprofv3
--kernel-trace --stats`, one profiled child process per measurement: the average duration per call over --repeats submits behind
one warm-up.  Per block: one child with -K all,5,5 and one with ds,5,5 (mask, gather, tally of that run); then --rounds times in
turn a child of this build with a record sink and no mask and, with --parent-lib, the same child on that library: select_gather
and the tally launch of each, every round listed, and the spread (smallest .. largest) of either side.  It measures and records;
it asserts only that every run kept what pss_ok counted and that the masked runs kept what the unmasked one kept."""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
FRACTIONS = (0.05, 0.5, 1.0)
MASKS = (("all", 5, 5), ("ds", 5, 5))


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
    return recs, offs, names, genome, region_len


def worker(a):
    """one engine with a record sink, one block, warm-up + repeats submits; prints one JSON line"""
    pkg = load_pkg(a.lib)
    recs, offs, names, genome, region_len = workload(pkg, a.worker, a.reads, a.scale_genome)
    eng = pkg.Engine(pss=dict(region_len=region_len))
    if a.fraction < 1.0:
        eng.set_regions(names, np.arange(len(names), dtype=np.int32), np.zeros(len(names), dtype=np.uint32),
                        np.array([max(1, int(g.size * a.fraction)) for _, g in genome], dtype=np.uint32))
    got = {"bytes": 0, "records": 0}

    def sink(chunk, n):
        got["bytes"] += chunk.size
        got["records"] += n

    eng.set_record_sink(sink)
    if a.mask:
        mode, n5, n3 = a.mask.split(",")
        eng.set_end_mask(mode, int(n5), int(n3))
    eng.set_genome_arrays(genome)
    eng.set_references(names)
    for _ in range(1 + a.repeats):
        eng.submit(recs, offs)
        eng.sync()
    st = eng.finish().stats
    eng.close()
    n_sub = 1 + a.repeats
    assert got["records"] == st["pss_ok"], (got, st)
    print("END_MASK_BENCH " + json.dumps({"workload": a.worker, "fraction_asked": a.fraction, "reads": a.reads, "block_bytes": int(offs[-1]),
                                          "kept_records": got["records"] // n_sub, "kept_bytes": got["bytes"] // n_sub,
                                          "fraction_kept": got["records"] / n_sub / a.reads}))


def profiled(a, name: str, fraction: float, lib: str | None, mask: str | None, tag: str, tmp: Path) -> dict:
    d = tmp / f"{name}_{fraction}_{tag}"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--", sys.executable, __file__,
           "--worker", name, "--fraction", str(fraction), "--reads", str(a.reads), "--repeats", str(a.repeats),
           "--scale-genome", str(a.scale_genome)] + (["--lib", lib] if lib else []) + (["--mask", mask] if mask else [])
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("END_MASK_BENCH ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(f"{' '.join(cmd)}\n{pr.stdout[-2000:]}\n{pr.stderr[-2000:]}")
    row = json.loads(line[0][len("END_MASK_BENCH "):])
    per_call = {}
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            per_call[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    n_sub = 1 + a.repeats

    def ms_per_submit(pred):
        return sum(t for k, (c, t) in per_call.items() if pred(k)) / n_sub / 1e6

    row["tally_ms"] = ms_per_submit(lambda k: "pssbam::tally_" in k or "pssbam::reduce_partials" in k)
    row["gather_ms"] = ms_per_submit(lambda k: "select_gather" in k)
    row["mask_ms"] = ms_per_submit(lambda k: "select_mask_ends" in k)
    row["select_launches_per_submit"] = sum(c for k, (c, _) in per_call.items() if "pssbam::select_" in k) / n_sub
    return row


def spread(v: list) -> dict:
    return {"rounds": v, "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--scale-genome", type=float, default=0.02)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "end_mask_bench.json"))
    ap.add_argument("--worker", default=None)            # (the profiled child)
    ap.add_argument("--fraction", type=float, default=1.0)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--mask", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rows = []
    with tempfile.TemporaryDirectory(prefix="end_mask_bench_") as td:
        tmp = Path(td)
        for name in ("C1", "C4"):
            for frac in FRACTIONS:
                row = {"workload": name, "fraction_asked": frac}
                for mode, n5, n3 in MASKS:
                    m = profiled(a, name, frac, None, f"{mode},{n5},{n3}", mode, tmp)
                    assert m["select_launches_per_submit"] == 6, m
                    row.update({k: m[k] for k in ("reads", "block_bytes", "kept_records", "kept_bytes", "fraction_kept")})
                    row[f"{mode}_{n5}_{n3}"] = {"mask_ms": m["mask_ms"], "gather_ms": m["gather_ms"], "tally_ms": m["tally_ms"],
                                                "mask_over_gather": m["mask_ms"] / m["gather_ms"], "mask_over_tally": m["mask_ms"] / m["tally_ms"]}
                sides = {"now": None, **({"parent": a.parent_lib} if a.parent_lib else {})}
                seen = {s: {"gather_ms": [], "tally_ms": []} for s in sides}
                for rnd in range(a.rounds):
                    for side, lib in sides.items():
                        u = profiled(a, name, frac, lib, None, f"{side}{rnd}", tmp)
                        assert u["kept_records"] == row["kept_records"] and u["select_launches_per_submit"] == 5 and u["mask_ms"] == 0, u
                        for k in seen[side]:
                            seen[side][k].append(u[k])
                row["unmasked"] = {s: {k: spread(v) for k, v in d.items()} for s, d in seen.items()}
                if a.parent_lib:
                    row["unmasked"]["ranges_overlap"] = {k: max(seen["now"][k]) >= min(seen["parent"][k]) and max(seen["parent"][k]) >= min(seen["now"][k])
                                                         for k in ("gather_ms", "tally_ms")}
                rows.append(row)
                print(json.dumps(row), flush=True)
    sec = {"statistic": "kernel ms per submit: rocprofv3 --kernel-trace --stats totals over 1 warm-up + repeats submits of one block, divided by "
                        "the submits; one profiled process per figure; unmasked: this build and the parent's library in turn, every round listed",
           "repeats": a.repeats, "rounds": a.rounds, "scale_genome": a.scale_genome, "parent_lib": bool(a.parent_lib), "blocks": rows}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    main()

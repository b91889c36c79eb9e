"""pss-bam -d cost: what duplicate flagging's kernels (insert, resolve, rehash, clear: csrc/dedup_kernels.h) take per submit beside
the tally launch they precede, and whether the tally launch with the setting off still takes what it took at the parent commit.

    python tools/dedup_bench.py [--reads 2000000] [--repeats 5] [--runs 3] [--scale-genome 0.02]
                                [--parent-lib <libpssbam_hip.so of the commit before the setting>] [--out profiles/dedup_bench.json]

Workloads: the synthetic C1 (100-base reads, one contig) and C4 (30..80-base reads, CIGAR mix, pre-flagged duplicates, low MAPQ)
records of bench.py's generator, one block of --reads records, as generated (0 % injected) and with the last 30 % of the records
replaced by copies of records drawn from the first 70 % (about 30 % injected; the engine's own count of flagged records is
recorded).  Kernel times come from `rocprofv3 --kernel-trace --stats`, one profiled child process per row: the total duration of
each kernel family over 1 warm-up + --repeats submits of the block -- the engine is reset in front of each, so every submit meets
an empty table of the size the first one grew it to -- divided by the submits.  The rehash is measured in a child of its own, once:
a table of 16 slots and the block in four quarters, so that the table doubles with keys in it; its row gives the calls and the
total.  With --parent-lib the setting-off tally launch is taken --runs times on each library, alternating; the file gives every
run and whether the two ranges overlap.  It measures and records; it asserts only that both libraries tallied the same reads."""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
INJECTED = (0.0, 0.3)
FAMILIES = {"insert_ms": "dedup_insert", "resolve_ms": "dedup_resolve", "rehash_ms": "dedup_rehash", "clear_ms": "dedup_clear"}


def load_pkg(lib: str | None):
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    if lib:
        pkg.LIB_HIP = Path(lib)
    return pkg


def workload(name: str, reads: int, scale: float, injected: float):
    from pss_bam_amd import synth
    d = synth.config(name, n_reads=reads, scale_genome=scale)
    region_len = d.pop("region_len")
    d.pop("klen", None)
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, reads, threads=16)
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(int(scfg.n_contigs))]
    if injected > 0:   # the last `injected` of the block becomes copies of records drawn from the part in front of it
        offs64 = offs.astype(np.int64)
        keep = reads - int(reads * injected)
        idx = np.concatenate([np.arange(keep), np.random.default_rng(1).integers(0, keep, size=reads - keep)])
        lens = (offs64[1:] - offs64[:-1])[idx]
        new_offs = np.concatenate([[0], np.cumsum(lens)])
        src = np.repeat(offs64[idx] - new_offs[:-1], lens) + np.arange(new_offs[-1])
        recs, offs = np.ascontiguousarray(recs[src]), new_offs.astype(np.uint32)
    return recs, offs, names, genome, region_len


def worker(a):
    """one engine, one block, warm-up + repeats submits behind a reset each; prints one JSON line"""
    pkg = load_pkg(a.lib)
    recs, offs, names, genome, region_len = workload(a.worker, a.reads, a.scale_genome, a.injected)
    eng = pkg.Engine(pss=dict(region_len=region_len))
    if a.mode != "off":
        eng.set_duplicates(True, 16 if a.mode == "growth" else 0)
    eng.set_genome_arrays(genome)
    eng.set_references(names)
    n = offs.size - 1
    n_sub = 1 if a.mode == "growth" else 1 + a.repeats
    cuts = [n * k // 4 for k in range(5)] if a.mode == "growth" else [0, n]
    totals = None
    for _ in range(n_sub):
        eng.reset()
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            o = offs[lo:hi + 1].astype(np.int64)
            eng.submit(recs[o[0]:o[-1]], (o - o[0]).astype(np.uint32))
        eng.sync()
        if a.mode != "off":
            totals = eng.finish_duplicates()[0]
    ms, launches = eng.kernel_time()
    st = eng.finish().stats
    eng.close()
    out = {"workload": a.worker, "mode": a.mode, "injected_asked": a.injected, "reads": n, "block_bytes": int(offs[-1]), "region_len": region_len,
           "submits": n_sub, "pss_ok": st["pss_ok"], "tally_launches_per_submit": launches / n_sub / (len(cuts) - 1), "duplicates": totals}
    print("DEDUP_BENCH " + json.dumps(out))


def profiled(a, name: str, injected: float, mode: str, lib: str | None, tmp: Path, tag: str) -> dict:
    d = tmp / f"{name}_{injected}_{mode}_{tag}"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--", sys.executable, __file__,
           "--worker", name, "--injected", str(injected), "--mode", mode, "--reads", str(a.reads), "--repeats", str(a.repeats),
           "--scale-genome", str(a.scale_genome)] + (["--lib", lib] if lib else [])
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("DEDUP_BENCH ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(f"{' '.join(cmd)}\n{pr.stdout[-2000:]}\n{pr.stderr[-2000:]}")
    row = json.loads(line[0][len("DEDUP_BENCH "):])
    per_call = {}
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            per_call[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    n_sub = row["submits"]
    pick = lambda pred: [(c, t) for k, (c, t) in per_call.items() if pred(k)]   # noqa: E731
    row["tally_ms"] = sum(t for _, t in pick(lambda k: "pssbam::tally_" in k or "pssbam::reduce_partials" in k)) / n_sub / 1e6
    if mode != "off":
        for key, kernel in FAMILIES.items():
            row[key] = sum(t for _, t in pick(lambda k: kernel in k)) / n_sub / 1e6
            row[key.replace("_ms", "_calls")] = sum(c for c, _ in pick(lambda k: kernel in k))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=0.02)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dedup_bench.json"))
    ap.add_argument("--worker", default=None)            # (the profiled child)
    ap.add_argument("--injected", type=float, default=0.0)
    ap.add_argument("--mode", default="on", choices=["on", "off", "growth"])
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rows, growth, off = [], [], []
    with tempfile.TemporaryDirectory(prefix="dedup_bench_") as td:
        tmp = Path(td)
        for name in ("C1", "C4"):
            for inj in INJECTED:
                row = profiled(a, name, inj, "on", None, tmp, "now")
                for k in ("insert", "resolve"):
                    row[f"{k}_over_tally"] = row[f"{k}_ms"] / row["tally_ms"]
                row["fraction_flagged"] = row["duplicates"]["flagged"] / row["reads"]
                rows.append(row)
                print(json.dumps(row), flush=True)
            g = profiled(a, name, 0.3, "growth", None, tmp, "now")
            growth.append(g)
            print(json.dumps(g), flush=True)
            runs = {"now": [], "parent": []}
            for k in range(a.runs):                      # alternating, so that drift of the machine shows in both
                for key, lib in (("now", None), ("parent", a.parent_lib)):
                    if key == "parent" and not lib:
                        continue
                    r = profiled(a, name, 0.0, "off", lib, tmp, f"{key}{k}")
                    runs[key].append(r)
            assert len({r["pss_ok"] for rr in runs.values() for r in rr}) == 1, runs
            ms = {k: [r["tally_ms"] for r in v] for k, v in runs.items() if v}
            entry = {"workload": name, "reads": a.reads, "tally_ms_setting_off": ms, "min": {k: min(v) for k, v in ms.items()},
                     "max": {k: max(v) for k, v in ms.items()}, "tally_launches_per_submit": runs["now"][0]["tally_launches_per_submit"]}
            if "parent" in ms:
                entry["ranges_overlap"] = max(ms["now"]) >= min(ms["parent"]) and max(ms["parent"]) >= min(ms["now"])
            off.append(entry)
            print(json.dumps(entry), flush=True)
    sec = {"statistic": "kernel ms per submit: rocprofv3 --kernel-trace --stats totals of a kernel family over 1 warm-up + repeats submits of one block "
                        "(a reset in front of each), divided by the submits; growth: one pass, a 16-slot table, the block in four quarters, "
                        "totals and calls as they are; setting off: the tally launch (tally kernel + its reduce) of `runs` processes per library, alternating",
           "repeats": a.repeats, "runs": a.runs, "scale_genome": a.scale_genome, "blocks": rows, "growth": growth, "setting_off": off}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    main()

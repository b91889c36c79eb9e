"""pss-bam -a cost: what allele_add (csrc/allele_kernels.h) takes per submit beside the tally launch it follows, for a sparse panel (one
site per 2500 bases, the density of a 1240k panel on a human genome) and a dense one (one per 100 bases), and whether the tally launch
with the setting off still takes what it took at the parent commit.

    python tools/allele_bench.py [--reads 2000000] [--repeats 5] [--runs 3] [--scale-genome 0.02]
                                 [--parent-lib <libpssbam_hip.so of the commit before the setting>] [--out profiles/allele_bench.json]

Blocks: the synthetic C1 (100-base reads, one contig) and C4 (30..80-base reads, CIGAR mix, duplicates, low MAPQ) records of bench.py's
generator, one block of --reads records sorted by (refID, POS).  Sites: every 2500th / every 100th position of every contig, from
position 7.  Kernel times come from `rocprofv3 --kernel-trace --stats`, one profiled child process per row: the total duration of each
kernel family over 1 warm-up + --repeats submits of the block (a reset in front of each), divided by the submits.  With --parent-lib the
setting-off tally launch is taken --runs times on each library, alternating; the file gives every run and whether the two ranges
overlap.  It measures and records; it asserts only that both libraries tallied the same reads."""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
PANELS = {"sparse": 2500, "dense": 100}


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
    n_sites = 0
    if a.mode == "on":
        step = PANELS[a.panel]
        pos = [np.arange(7, g.size, step, dtype=np.uint32) for _, g in genome]
        n_sites = int(sum(p.size for p in pos))
        eng.set_sites(names, np.concatenate([np.full(p.size, k, dtype=np.int32) for k, p in enumerate(pos)]), np.concatenate(pos))
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
        ref, pos0, base, counts, totals = eng.finish_sites()
        cov = {"panel": a.panel, "site_every": PANELS[a.panel], "sites": n_sites, "genome_positions": int(sum(g.size for _, g in genome)), **totals,
               "max_depth": int(counts.astype(np.int64).sum(axis=1).max())}
    st = eng.finish().stats
    eng.close()
    print("ALLELE_BENCH " + json.dumps({"workload": a.worker, "order": a.order, "mode": a.mode, "reads": int(offs.size - 1), "block_bytes": int(offs[-1]),
                                          "region_len": region_len, "submits": n_sub, "pss_ok": st["pss_ok"], "tally_launches_per_submit": launches / n_sub,
                                          "alleles": cov}))


def profiled(a, args: list, lib: str | None, tmp: Path, tag: str):
    d = tmp / tag
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(d), "--", sys.executable, __file__, *args, "--reads", str(a.reads),
           "--repeats", str(a.repeats), "--scale-genome", str(a.scale_genome)] + (["--lib", lib] if lib else [])
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
    line = [ln for ln in pr.stdout.splitlines() if ln.startswith("ALLELE_BENCH ")]
    if pr.returncode != 0 or not line:
        raise RuntimeError(f"{' '.join(cmd)}\n{pr.stdout[-2000:]}\n{pr.stderr[-2000:]}")
    row = json.loads(line[0][len("ALLELE_BENCH "):])
    per_call = {}
    for f in d.rglob("*kernel_stats.csv"):
        for r in csv.DictReader(open(f)):
            per_call[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]))
    return row, (lambda pred: [(c, t) for k, (c, t) in per_call.items() if pred(k)])


def block_row(a, name, order, mode, lib, tmp, tag, panel="sparse"):
    row, pick = profiled(a, ["--worker", name, "--order", order, "--mode", mode, "--panel", panel], lib, tmp, f"{name}_{order}_{mode}_{panel}_{tag}")
    row["tally_ms"] = sum(t for _, t in pick(lambda k: "pssbam::tally_" in k or "pssbam::reduce_partials" in k)) / row["submits"] / 1e6
    if mode == "on":
        row["allele_add_ms"] = sum(t for _, t in pick(lambda k: "allele_add" in k)) / row["submits"] / 1e6
        row["allele_add_over_tally"] = row["allele_add_ms"] / row["tally_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=0.02)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "allele_bench.json"))
    ap.add_argument("--worker", default=None)            # (the profiled child: a workload's name)
    ap.add_argument("--panel", default="sparse", choices=list(PANELS))
    ap.add_argument("--order", default="sorted", choices=["sorted", "shuffled"])
    ap.add_argument("--mode", default="on", choices=["on", "off"])
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.worker:
        return block_worker(a)
    rows, off = [], []
    with tempfile.TemporaryDirectory(prefix="allele_bench_") as td:
        tmp = Path(td)
        for name in ("C1", "C4"):
            for panel in PANELS:
                row = block_row(a, name, "sorted", "on", None, tmp, "now", panel)
                rows.append(row)
                print(json.dumps(row), flush=True)
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
    sec = {"statistic": "kernel ms per submit, rocprofv3 --kernel-trace --stats totals of a kernel family over 1 warm-up + repeats submits of one block "
                        "(a reset in front of each), divided by the submits; tally = the tally kernel + its reduce; setting off: the tally launch of "
                        "`runs` processes per library, alternating",
           "repeats": a.repeats, "runs": a.runs, "scale_genome": a.scale_genome, "blocks": rows, "setting_off": off}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    main()

"""pss-bam -T cost: tally-kernel time of C4-shaped (30-80 bp, N = 15) synthetic records over the synthetic genome, for
    unfiltered AUTO, unfiltered TILED, -T with one interval per contig that covers everything, -T with 1 k and with 200 k
    evenly tiled intervals that keep about half the reads, the 200 k leg with -S on 4 edges, and the 200 k leg with the
    lookup grid bypassed (PSSBAM_REGION_GRID_SHIFT at its maximum: one grid word per 2^20 bases, the search inside a bin
    is then a plain binary search over its intervals).

    python tools/region_bench.py [--reads 4000000] [--runs 7] [--scale-genome 0.05] [--out profiles/region_bench.json]
                                 [--baseline-only] [--parent-json FILE]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included; every leg tallies
the same records.  The legs alternate: each of --runs rounds times every leg once (a fresh engine each), and a leg's
figure is the median over the rounds.  --baseline-only runs just the two unfiltered legs and uses nothing of the -T
interface, so the same file can be run from a checkout of the commit before -T; --parent-json merges that run's output
in, and every -T leg is then also reported as a ratio to the parent's unfiltered TILED leg -- the yardstick, since -T
runs on tally_tiled for every -r.  No ratio is judged here."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

EDGES = [40, 50, 60, 70]


def tiled_intervals(lens: list, n: int):
    """n intervals spread evenly over the contigs (by length), each covering the first half of its period"""
    total = float(sum(lens))
    name_of, starts, ends = [], [], []
    for k, ln in enumerate(lens):
        m = max(1, int(round(n * ln / total)))
        period = ln / m
        s = (np.arange(m) * period).astype(np.int64)
        name_of.append(np.full(m, k, dtype=np.int32))
        starts.append(s)
        ends.append(np.minimum(s + max(1, int(period / 2)), ln))
    return np.concatenate(name_of), np.concatenate(starts).astype(np.uint32), np.concatenate(ends).astype(np.uint32)


def stat(xs: list) -> dict:
    return {"runs_ms": xs, "min_ms": min(xs), "max_ms": max(xs), "median_ms": float(np.median(xs)),
            "spread_rel": (max(xs) - min(xs)) / min(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--scale-genome", type=float, default=0.05)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "region_bench.json"))
    a = ap.parse_args()
    pkg = ge.load_pkg()
    from pss_bam_amd import synth
    d = synth.config("C4", n_reads=a.reads, scale_genome=a.scale_genome)
    region_len = d.pop("region_len")
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]
    lens = [int(g.size) for _, g in genome]
    gnames = [nm for nm, _ in genome]

    def engine(kernel=pkg.KERNEL_AUTO, regions=None, shift=None, **kw):
        if shift is None:
            os.environ.pop("PSSBAM_REGION_GRID_SHIFT", None)
        else:
            os.environ["PSSBAM_REGION_GRID_SHIFT"] = str(shift)   # read when the engine is created
        eng = pkg.Engine(pss=dict(region_len=region_len), kernel=kernel, **kw)
        if regions is not None:
            eng.set_regions(gnames, *regions)
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        return eng

    def timed(eng):
        eng.kernel_time(reset=True)
        eng.submit(recs, offs)            # the first submit sizes the staging and warms the launch up
        eng.sync()
        eng.kernel_time(reset=True)
        eng.reset()
        eng.submit(recs, offs)
        eng.sync()
        ms, _ = eng.kernel_time(reset=True)
        return ms

    legs = {"unfiltered_AUTO": dict(kernel=pkg.KERNEL_AUTO), "unfiltered_TILED": dict(kernel=pkg.KERNEL_TILED)}
    if not a.baseline_only:
        cover = (np.arange(len(lens), dtype=np.int32), np.zeros(len(lens), dtype=np.uint32), np.array(lens, dtype=np.uint32))
        t1k, t200k = tiled_intervals(lens, 1000), tiled_intervals(lens, 200_000)
        legs.update({"T_cover_everything": dict(regions=cover), "T_1k_intervals": dict(regions=t1k),
                     "T_200k_intervals": dict(regions=t200k), "T_200k_intervals_S_4_edges": dict(regions=t200k, length_bins=EDGES),
                     "T_200k_intervals_grid_bypassed": dict(regions=t200k, shift=20)})
    runs = {k: [] for k in legs}
    tables = {}
    for _ in range(a.runs):
        for name, kw in legs.items():
            eng = engine(**kw)
            runs[name].append(timed(eng))
            if name not in tables:
                t = eng.finish()
                tables[name] = (t.fwd, t.rev, t.stats)
            eng.close()
    res = {"reads": a.reads, "runs": a.runs, "scale_genome": a.scale_genome, "shape": "C4", "region_len": region_len,
           "record_bytes_mean": float(offs[-1]) / a.reads, "genome_bases": int(sum(lens)), "contigs": len(lens),
           "statistic": "median over alternating rounds, tally kernels only (Engine.kernel_time), second submit of a fresh engine",
           "baseline_only": a.baseline_only, "legs": {k: stat(v) for k, v in runs.items()}}
    ms = {k: v["median_ms"] for k, v in res["legs"].items()}
    res["reads_per_s"] = {k: a.reads / (v * 1e-3) for k, v in ms.items()}
    if not a.baseline_only:
        un = tables["unfiltered_TILED"]
        res["checks"] = {
            "cover_everything_tables_equal_unfiltered": bool(np.array_equal(tables["T_cover_everything"][0], un[0]) and
                                                             np.array_equal(tables["T_cover_everything"][1], un[1])),
            "grid_bypassed_tables_equal_grid": bool(np.array_equal(tables["T_200k_intervals_grid_bypassed"][0], tables["T_200k_intervals"][0])),
            "kept_fraction": {k: tables[k][2]["pss_ok"] / max(un[2]["pss_ok"], 1) for k in tables if k.startswith("T_")}}
        res["ratio_to_unfiltered_TILED_this_commit"] = {k: ms[k] / ms["unfiltered_TILED"] for k in ms if k.startswith("T_")}
        res["grid_vs_bypassed"] = {"grid_ms": ms["T_200k_intervals"], "bypassed_ms": ms["T_200k_intervals_grid_bypassed"],
                                   "grid_wins": bool(ms["T_200k_intervals"] <= ms["T_200k_intervals_grid_bypassed"])}
    if a.parent_json:
        parent = json.loads(Path(a.parent_json).read_text())
        pm = parent["legs"]["unfiltered_TILED"]["median_ms"]
        res["parent"] = {"legs": parent["legs"], "yardstick": "the parent commit's unfiltered TILED leg, same records",
                         "ratio_to_parent_unfiltered_TILED": {k: v / pm for k, v in ms.items()}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""fragkon -S cost: tally-kernel time of C4-shaped records (30-80 bp damaged reads) through a k-mer engine, k = 4 (LDS
histograms per plane) and k = 8 (global atomics), for
  * one unbinned run,
  * the only way to per-bin tables without planes: one unbinned run per bin with -l / -L set to the bin, times summed,
  * one binned pass with 4 edges (5 bins) and with 63 edges (64 bins).

    python tools/kmer_planes_bench.py [--reads 4000000] [--repeats 7] [--scale-genome 1.0] [--out profiles/kmer_planes_bench.json]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included.  Every leg
tallies the same resident records.  All engines of one k are built first; after one warm-up submit each, the legs
alternate inside every repeat, and the statistic is the median over the repeats.  Required: the 5-bin pass takes
less kernel time than the five windowed runs together (it reads the records once instead of five times).  The 64
windowed runs are only timed with --full (64 more engines); the 64-bin pass is always timed."""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

EDGES = {"S_5bins": [40, 50, 60, 70], "S_64bins": list(range(18, 81))}   # the C4 reads are 30-80 bp


def windows(edges):
    return list(zip([0] + edges, [e - 1 for e in edges] + [250000000]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--full", action="store_true", help="also time the 64 windowed runs of the 64-bin case")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "kmer_planes_bench.json"))
    a = ap.parse_args()
    pkg = ge.load_pkg()
    from pss_bam_amd import synth
    d = synth.config("C4", n_reads=a.reads, scale_genome=a.scale_genome)
    d.pop("region_len")
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]

    def engine(k, edges=None, **kmer):
        eng = pkg.Engine(kmer=dict(klen=k, **kmer), length_bins=edges)
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        return eng

    def run(eng) -> float:
        eng.submit(recs, offs)
        eng.sync()
        return eng.kernel_time(reset=True)[0]

    res = {"reads": a.reads, "record_bytes_mean": float(offs[-1]) / a.reads, "repeats": a.repeats,
           "statistic": "median over repeats of the tally kernels' time (Engine.kernel_time), legs alternating inside every "
                        "repeat after one warm-up submit per engine",
           "edges": EDGES, "k": {}}
    for k in (4, 8):
        legs = {"unbinned": [engine(k)]}
        legs["windows_5"] = [engine(k, min_read_len=lo, max_read_len=hi) for lo, hi in windows(EDGES["S_5bins"])]
        for name, edges in EDGES.items():
            legs[name] = [engine(k, edges=edges)]
        if a.full:
            legs["windows_64"] = [engine(k, min_read_len=lo, max_read_len=hi) for lo, hi in windows(EDGES["S_64bins"])]
        for engs in legs.values():               # warm-up: first launches, scratch and prefix sampling
            for eng in engs:
                run(eng)
                eng.reset()
        samples = {name: [] for name in legs}
        for _ in range(a.repeats):
            for name, engs in legs.items():
                samples[name].append(sum(run(eng) for eng in engs))
        ms = {name: statistics.median(v) for name, v in samples.items()}
        want = legs["unbinned"][0].finish()
        out = {"ms": ms, "ms_samples": samples, "bins_sum_to_unbinned": {}}
        for name in EDGES:
            got = legs[name][0].finish_bins()
            out["bins_sum_to_unbinned"][name] = bool(np.array_equal(sum(t.k5 for t in got.values()), want.k5) and
                                                     np.array_equal(sum(t.k3 for t in got.values()), want.k3))
        out["ratio_5bins_over_five_windowed_runs"] = ms["S_5bins"] / ms["windows_5"]
        out["ratio_5bins_over_unbinned"] = ms["S_5bins"] / ms["unbinned"]
        out["ratio_64bins_over_unbinned"] = ms["S_64bins"] / ms["unbinned"]
        if a.full:
            out["ratio_64bins_over_64_windowed_runs"] = ms["S_64bins"] / ms["windows_64"]
        out["required_5bins_faster_than_five_windowed_runs"] = ms["S_5bins"] < ms["windows_5"]
        out["reads_per_s"] = {name: a.reads / (v * 1e-3) for name, v in ms.items()}
        res["k"][str(k)] = out
        for engs in legs.values():
            for eng in engs:
                eng.close()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: {x: v[x] for x in v if x.startswith("ratio") or x.startswith("required") or x == "ms"}
                      for k, v in res["k"].items()}))


if __name__ == "__main__":
    main()

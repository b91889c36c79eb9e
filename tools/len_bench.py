"""pss-bam -S cost: tally-kernel time of C4-shaped records (30-80 bp damaged reads, N = 15) for the unbinned run
(KERNEL_AUTO = tally_compact, and KERNEL_TILED), one -l / -L window, and -S with 1, 4, 9 and 63 edges.

    python tools/len_bench.py [--reads 4000000] [--repeats 5] [--scale-genome 1.0] [--out profiles/len_bench.json]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included.  Every
run tallies the same records.  Targets: -S with 4 edges (5 bins) at most 1.5x the unbinned AUTO run and at
most 1.25x the unbinned TILED run."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

EDGES = {
    "S_1": [55],
    "S_4": [40, 50, 60, 70],
    "S_9": list(range(35, 80, 5)),
    "S_63": list(range(18, 81)),      # 64 bins + plane 0: more planes than one launch's LDS holds
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "len_bench.json"))
    a = ap.parse_args()
    pkg = ge.load_pkg()
    from pss_bam_amd import synth
    d = synth.config("C4", n_reads=a.reads, scale_genome=a.scale_genome)
    region_len = d.pop("region_len")
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    n_contigs = int(scfg.n_contigs)
    names = [synth.contig_name(scfg, k) for k in range(n_contigs)]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]

    def engine(kernel=pkg.KERNEL_AUTO, edges=None, **pss):
        eng = pkg.Engine(pss=dict(region_len=region_len, **pss), kernel=kernel, length_bins=edges)
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        return eng

    def timed(eng) -> float:
        best = None
        eng.kernel_time(reset=True)
        for _ in range(a.repeats):
            eng.submit(recs, offs)
            eng.sync()
            ms, _ = eng.kernel_time(reset=True)
            best = ms if best is None else min(best, ms)
        return best

    res = {"reads": a.reads, "region_len": region_len, "record_bytes_mean": float(offs[-1]) / a.reads,
           "repeats": a.repeats, "statistic": "best of repeats, tally kernels only (Engine.kernel_time)",
           "edges": EDGES, "ms": {}, "bins_sum_to_unbinned": {}}
    eng = engine()
    res["ms"]["unbinned_AUTO"] = timed(eng)
    eng.close()
    eng = engine(pkg.KERNEL_TILED)
    res["ms"]["unbinned_TILED"] = timed(eng)
    want = eng.finish()
    eng.close()
    eng = engine(min_read_len=40, max_read_len=49)
    res["ms"]["one_l_L_window"] = timed(eng)
    eng.close()
    for name, edges in EDGES.items():
        eng = engine(edges=edges)
        res["ms"][name] = timed(eng)
        got = eng.finish_bins()
        res["bins_sum_to_unbinned"][name] = bool(np.array_equal(sum(t.fwd for t in got.values()), want.fwd) and
                                                 np.array_equal(sum(t.rev for t in got.values()), want.rev))
        eng.close()
    ms = res["ms"]
    res["ratio_S4_over_AUTO"] = ms["S_4"] / ms["unbinned_AUTO"]
    res["ratio_S4_over_TILED"] = ms["S_4"] / ms["unbinned_TILED"]
    res["ratio_five_l_L_runs_over_AUTO"] = 5 * ms["one_l_L_window"] / ms["unbinned_AUTO"]
    res["target_S4_le_1.5x_AUTO"] = res["ratio_S4_over_AUTO"] <= 1.5
    res["target_S4_le_1.25x_TILED"] = res["ratio_S4_over_TILED"] <= 1.25
    res["reads_per_s"] = {k: a.reads / (v * 1e-3) for k, v in ms.items()}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

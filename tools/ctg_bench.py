"""pss-bam -C cost: tally-kernel time of C4-shaped records (30-80 bp damaged reads, N = 15, over the synthetic
genome's contigs) for the unsplit run (KERNEL_AUTO = tally_compact, and KERNEL_TILED), -S with 4 edges (5 planes),
and -C with {chrX}, with {chrX}, {chrY}, {chr1-11}, {chr12-22} (5 planes, as many as -S 4) and with one set per
contig (25 planes: more than one plane pass).

    python tools/ctg_bench.py [--reads 4000000] [--repeats 5] [--scale-genome 1.0] [--out profiles/ctg_bench.json]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included.  Every
run tallies the same records.  Target: -C with 4 sets at most 1.05x the -S 4-edge run."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ctg_bench.json"))
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
    sets = {
        "C_chrX": {"X": ["chrX"]},
        "C_4": {"X": ["chrX"], "Y": ["chrY"], "1-11": [f"chr{i}" for i in range(1, 12)],
                "12-22": [f"chr{i}" for i in range(12, 23)]},
        "C_per_contig": {nm: [nm] for nm in names},
    }
    missing = sorted({nm for s in sets.values() for v in s.values() for nm in v} - set(names))
    if missing:
        raise SystemExit(f"the synthetic genome lacks {missing}: contigs are {names}")

    def engine(kernel=pkg.KERNEL_AUTO, **planes):
        eng = pkg.Engine(pss=dict(region_len=region_len), kernel=kernel, **planes)
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
           "contigs": names, "repeats": a.repeats, "statistic": "best of repeats, tally kernels only (Engine.kernel_time)",
           "sets": {k: list(v) for k, v in sets.items()}, "ms": {}, "sets_plus_unassigned_sum_to_unsplit": {}}
    eng = engine()
    res["ms"]["unsplit_AUTO"] = timed(eng)
    eng.close()
    eng = engine(pkg.KERNEL_TILED)
    res["ms"]["unsplit_TILED"] = timed(eng)
    want = eng.finish()
    eng.close()
    eng = engine(length_bins=[40, 50, 60, 70])
    res["ms"]["S_4"] = timed(eng)
    eng.close()
    for name, s in sets.items():
        eng = engine(contig_sets=s)
        res["ms"][name] = timed(eng)
        got = eng.finish_sets()
        p0f = np.zeros((region_len + 2, 16), dtype=np.uint64)
        p0r = np.zeros_like(p0f)
        assert eng._L.pssbam_engine_finish_groups(eng._h, -1, p0f.ctypes.data, p0r.ctypes.data) == 0
        res["sets_plus_unassigned_sum_to_unsplit"][name] = bool(
            np.array_equal(sum(t.fwd for t in got.values()) + p0f, want.fwd) and
            np.array_equal(sum(t.rev for t in got.values()) + p0r, want.rev))
        eng.close()
    ms = res["ms"]
    res["ratio_C4_over_S4"] = ms["C_4"] / ms["S_4"]
    res["ratio_C4_over_AUTO"] = ms["C_4"] / ms["unsplit_AUTO"]
    res["target_C4_le_1.05x_S4"] = res["ratio_C4_over_S4"] <= 1.05
    res["reads_per_s"] = {k: a.reads / (v * 1e-3) for k, v in ms.items()}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""pss-bam -J cost: tally-kernel time of C2-shaped records (<150>M reads over the synthetic genome) at N = 15 for
    unsplit_TILED   the unsplit run, KERNEL_TILED
    S_6             -S with 5 edges: 6 bins and plane 0
    J_6             -J 6: the same number of planes and plane passes, the plane picked by the read-name hash
    S_20            -S with 19 edges: 20 bins and plane 0
    J_20            -J 20

    python tools/replicates_bench.py [--reads 4000000] [--rounds 7] [--out profiles/replicates_bench.json]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included.  All legs are
measured in one session, a warm-up round first and then `rounds` rounds that visit the legs in turn, so a drift of the
machine meets every leg alike.  A leg's figure is the median of its rounds.  No ratio is fixed in advance: the yardsticks
are the two -S legs -- the code without the setting, with the same planes and passes -- and each -J leg is reported as a
ratio to its -S leg next to that leg's own spread over the rounds (min / median .. max / median).
(tally_launches_per_submit: the intervals Engine.kernel_time timed -- one per submit, whatever the passes inside it.)"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

EDGES = {6: [30, 60, 90, 120, 140], 20: list(range(7, 140, 7))}   # every <150>M read lands in the last bin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "replicates_bench.json"))
    a = ap.parse_args()
    pkg = ge.load_pkg()
    from pss_bam_amd import synth
    d = synth.config("C2", n_reads=a.reads, scale_genome=a.scale_genome)
    d.pop("region_len")
    region_len = 15
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]
    name_len = int(recs[12]) - 1
    print(f"records and genome ready: {a.reads} reads over {last_contig + 1} of {len(names)} contigs, read names of {name_len} bytes", flush=True)

    def engine(**kw):
        eng = pkg.Engine(pss=dict(region_len=region_len), kernel=pkg.KERNEL_TILED, **kw)
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        return eng

    legs = {"unsplit_TILED": engine()}
    for k, edges in EDGES.items():
        assert len(edges) == k - 1
        legs[f"S_{k}"] = engine(length_bins=edges)
        legs[f"J_{k}"] = engine(replicates=k)
    times = {k: [] for k in legs}
    launches = {}
    for rnd in range(a.rounds + 1):             # round 0 warms every leg up
        for name, eng in legs.items():
            eng.reset()
            eng.kernel_time(reset=True)
            eng.submit(recs, offs)
            eng.sync()
            ms, n = eng.kernel_time(reset=True)
            launches[name] = n
            if rnd:
                times[name].append(ms)
        print(f"round {rnd} done", flush=True)
    want = legs["unsplit_TILED"].finish()
    same, per_plane = {}, {}
    for name, eng in legs.items():
        tot = eng.finish()
        ok = np.array_equal(tot.fwd, want.fwd) and np.array_equal(tot.rev, want.rev)
        if name.startswith("J_"):
            fwd, rev = eng.finish_replicates()
            ok = ok and np.array_equal(fwd.sum(axis=0), want.fwd) and np.array_equal(rev.sum(axis=0), want.rev)
            per_plane[name] = [int(x) for x in fwd[:, 2].sum(axis=1)]          # reads per replicate in the forward table (row 0 of the positions)
        same[name] = bool(ok)
        eng.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    spread = {k: [min(v) / med[k], max(v) / med[k]] for k, v in times.items()}
    res = {"reads": a.reads, "region_len": region_len, "record_bytes_mean": float(offs[-1]) / a.reads, "read_name_bytes": name_len,
           "rounds": a.rounds,
           "statistic": "median of rounds, tally kernels only (Engine.kernel_time); legs visited in turn, one warm-up round; "
                        "spread = [min / median, max / median] over the rounds",
           "edges": {f"S_{k}": e for k, e in EDGES.items()}, "tally_launches_per_submit": launches,
           "ms": med, "spread": spread, "all_ms": times, "tables_equal_unsplit": same, "forward_reads_per_replicate": per_plane,
           "ratio_J_over_S": {str(k): med[f"J_{k}"] / med[f"S_{k}"] for k in EDGES},
           "ratio_to_unsplit": {k: v / med["unsplit_TILED"] for k, v in med.items()},
           "reads_per_s": {k: a.reads / (v * 1e-3) for k, v in med.items()}}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "all_ms"}))
    if not all(same.values()):
        raise SystemExit(1)


if __name__ == "__main__":
    main()

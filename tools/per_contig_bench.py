"""pss-bam -A cost: tally-kernel time of C4-shaped records (30-80 bp damaged reads, N = 15, over the synthetic genome's
contigs) for
    unsplit_TILED     the unsplit run, KERNEL_TILED
    C_per_contig      -C with one set per contig (the only way to get every contig's tables before -A)
    A_sorted          -A on the same, coordinate-sorted records
    A_shuffled        -A on the same records in random order: every tile mixes contigs, misses dominate
    A_shuffled_S1     the same with PSSBAM_CONTIG_SLOTS=1, the worst case
and, beside them, A_sorted with other slot counts (--sweep) and with PSSBAM_CONTIG_EVICT=0 (slots emptied at a miss only).

    python tools/per_contig_bench.py [--reads 4000000] [--repeats 5] [--out profiles/per_contig_bench.json]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included.  All rows are
measured in one session, a warm-up round first and then `repeats` rounds that visit the rows in turn, so a drift of
the machine meets every row alike.  A row's figure is the best of its repeats; its spread is median - best.
Acceptance: A_sorted <= C_per_contig + the larger of the two rows' spreads."""
import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402


def shuffled(recs: np.ndarray, offs: np.ndarray, seed: int):
    """the same records in random order (chunked gather: the byte index of a whole block would not fit)"""
    n = offs.size - 1
    perm = np.random.default_rng(seed).permutation(n)
    lens = np.diff(offs.astype(np.int64))
    out = np.empty_like(recs)
    new_offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens[perm], out=new_offs[1:])
    for lo in range(0, n, 200_000):
        idx = perm[lo:lo + 200_000]
        ln = lens[idx]
        dst0 = new_offs[lo]
        pos = np.cumsum(ln) - ln
        src = np.repeat(offs[idx].astype(np.int64) - pos, ln) + np.arange(int(ln.sum()), dtype=np.int64)
        out[dst0:dst0 + src.size] = recs[src]
    return out, new_offs.astype(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--sweep", default="1,3,15", help="slot counts of the extra A_sorted rows ('' = none)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "per_contig_bench.json"))
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
    print(f"records and genome ready: {a.reads} reads over {last_contig + 1} of {len(names)} contigs", flush=True)
    recs_sh, offs_sh = shuffled(recs, offs, 1)
    print("shuffled copy ready", flush=True)

    def engine(slots=None, evict=True, **kw):
        if slots is None:
            os.environ.pop("PSSBAM_CONTIG_SLOTS", None)
        else:
            os.environ["PSSBAM_CONTIG_SLOTS"] = str(slots)      # (read when the engine is created)
        os.environ["PSSBAM_CONTIG_EVICT"] = "1" if evict else "0"   # (likewise)
        eng = pkg.Engine(pss=dict(region_len=region_len), kernel=pkg.KERNEL_TILED, **kw)
        os.environ.pop("PSSBAM_CONTIG_SLOTS", None)
        os.environ.pop("PSSBAM_CONTIG_EVICT", None)
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        return eng

    rows = {
        "unsplit_TILED": (engine(), recs, offs),
        "C_per_contig": (engine(contig_sets={nm: [nm] for nm in names}), recs, offs),
        "A_sorted": (engine(per_contig=True), recs, offs),
        "A_shuffled": (engine(per_contig=True), recs_sh, offs_sh),
        "A_shuffled_S1": (engine(slots=1, per_contig=True), recs_sh, offs_sh),
    }
    for s in [int(x) for x in a.sweep.split(",") if x]:
        rows[f"A_sorted_S{s}"] = (engine(slots=s, per_contig=True), recs, offs)
    rows["A_sorted_no_evict"] = (engine(evict=False, per_contig=True), recs, offs)   # A/B: slots are emptied at a miss only
    times = {k: [] for k in rows}
    for rep in range(a.repeats + 1):            # round 0 warms every row up
        for name, (eng, r, o) in rows.items():
            eng.reset()
            eng.kernel_time(reset=True)
            eng.submit(r, o)
            eng.sync()
            ms, _ = eng.kernel_time(reset=True)
            if rep:
                times[name].append(ms)
        print(f"round {rep} done", flush=True)
    want = rows["unsplit_TILED"][0].finish()
    same = {}
    for name, (eng, _, _) in rows.items():
        if name.startswith("A_"):
            got, tot = eng.finish_contigs(), eng.finish()
            same[name] = bool(np.array_equal(tot.fwd, want.fwd) and np.array_equal(tot.rev, want.rev) and
                              np.array_equal(sum(t.fwd for t in got.values()), want.fwd) and
                              {k: v for k, v in tot.stats.items() if k != "slow_path"} == {k: v for k, v in want.stats.items() if k != "slow_path"})
            touched = len(got)
        eng.close()
    best = {k: min(v) for k, v in times.items()}
    spread = {k: float(np.median(v)) - min(v) for k, v in times.items()}
    margin = max(spread["A_sorted"], spread["C_per_contig"])
    res = {"reads": a.reads, "region_len": region_len, "record_bytes_mean": float(offs[-1]) / a.reads, "contigs_with_reads": last_contig + 1,
           "contigs_in_header": len(names), "touched_planes": touched, "repeats": a.repeats,
           "statistic": "best of repeats, tally kernels only (Engine.kernel_time); rows visited in turn, one warm-up round; spread = median - best",
           "ms": best, "spread_ms": spread, "all_ms": times, "planes_sum_to_unsplit_and_stats_equal": same,
           "ratio_to_unsplit": {k: v / best["unsplit_TILED"] for k, v in best.items()},
           "reads_per_s": {k: a.reads / (v * 1e-3) for k, v in best.items()},
           "margin_ms": margin, "A_sorted_le_C_per_contig_plus_margin": bool(best["A_sorted"] <= best["C_per_contig"] + margin)}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if k != "all_ms"}))
    if not all(same.values()) or not res["A_sorted_le_C_per_contig_plus_margin"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()

"""pss-bam -Q cost: tally-kernel time of C3-shaped (150 bp, N = 25) and C4-shaped (30-80 bp, N = 15) records whose
QUAL bytes are seeded random Phred 2..41 and which all carry RG:Z:L000, for
    unmasked AUTO, unmasked TILED, -R L000 (keeps every record: the existing whole-record path), -Q 20, -Q 20 -S (4 edges).

    python tools/bq_bench.py [--reads 2000000] [--repeats 5] [--runs 5] [--scale-genome 0.05] [--out profiles/bq_bench.json]
                             [--baseline-only] [--parent-json FILE]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included; every leg
tallies the same records.  The two unmasked legs are run --runs times (a fresh engine each, best of --repeats); their
spread is recorded.  --baseline-only runs just those two legs and uses nothing of the -Q interface, so the same file
can be run from a checkout of the commit before -Q; --parent-json merges that run's output in, and the unmasked legs
of this commit are then judged against the parent's: the allowed difference is the parent's own run-to-run spread.
The cost of -Q itself is reported as the ratio to the -R leg (same staging, plus one LDS fetch and a few VALU
operations per lane) and to unmasked AUTO, without a threshold."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import __graft_entry__ as ge  # noqa: E402
from rg_bench import with_rg  # noqa: E402

EDGES = {"C3": [40, 80, 120, 150], "C4": [40, 50, 60, 70]}


def random_quals(recs: np.ndarray, offs: np.ndarray, seed: int, chunk: int = 1 << 16) -> None:
    """overwrites every record's QUAL bytes with seeded random Phred 2..41"""
    rng = np.random.default_rng(seed)
    n = offs.size - 1
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        o = offs[a:b].astype(np.int64)
        l_name = recs[o + 12].astype(np.int64)
        n_cig = recs[o + 16].astype(np.int64) | (recs[o + 17].astype(np.int64) << 8)
        l_seq = sum(recs[o + 20 + k].astype(np.int64) << (8 * k) for k in range(4))
        q0 = o + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2
        first = np.cumsum(l_seq) - l_seq
        idx = np.repeat(q0 - first, l_seq) + np.arange(int(l_seq.sum()), dtype=np.int64)
        recs[idx] = rng.integers(2, 42, size=idx.size, dtype=np.uint8)


def spread(xs: list) -> dict:
    return {"runs_ms": xs, "min_ms": min(xs), "max_ms": max(xs), "median_ms": float(np.median(xs)),
            "spread_rel": (max(xs) - min(xs)) / min(xs)}


def bench_shape(pkg, synth, shape: str, a) -> dict:
    d = synth.config(shape, n_reads=a.reads, scale_genome=a.scale_genome)
    region_len = d.pop("region_len")
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]
    recs, offs, val_at = with_rg(recs, offs)
    for k, byte in enumerate(b"L000"):
        recs[val_at + k] = byte
    random_quals(recs, offs, seed=20 + len(shape))

    def engine(kernel=pkg.KERNEL_AUTO, **kw):
        eng = pkg.Engine(pss=dict(region_len=region_len), kernel=kernel, **kw)
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

    res = {"region_len": region_len, "record_bytes_mean": float(offs[-1]) / a.reads, "ms": {}}
    runs = {"unmasked_AUTO": [], "unmasked_TILED": []}
    want = None
    for _ in range(a.runs):
        for name, kernel in (("unmasked_AUTO", pkg.KERNEL_AUTO), ("unmasked_TILED", pkg.KERNEL_TILED)):
            eng = engine(kernel)
            runs[name].append(timed(eng))
            if want is None:
                want = eng.finish()
            eng.close()
    res["unmasked_runs"] = {k: spread(v) for k, v in runs.items()}
    res["ms"]["unmasked_AUTO"], res["ms"]["unmasked_TILED"] = min(runs["unmasked_AUTO"]), min(runs["unmasked_TILED"])
    if a.baseline_only:
        return res
    eng = engine(read_group="L000")
    res["ms"]["R_keeps_every_record"] = timed(eng)
    got = eng.finish()
    res["R_tables_equal_unmasked"] = bool(np.array_equal(got.fwd, want.fwd) and np.array_equal(got.rev, want.rev))
    eng.close()
    eng = engine(min_base_qual=0)
    timed(eng)
    got = eng.finish()
    res["Q0_tables_equal_unmasked"] = bool(np.array_equal(got.fwd, want.fwd) and np.array_equal(got.rev, want.rev))
    eng.close()
    eng = engine(min_base_qual=20)
    res["ms"]["Q20"] = timed(eng)
    q20 = eng.finish()
    res["Q20_tables_differ"] = bool((q20.fwd[2:] != want.fwd[2:]).any() and (q20.rev[2:] != want.rev[2:]).any())
    res["Q20_context_rows_equal_unmasked"] = bool(np.array_equal(q20.fwd[:2], want.fwd[:2]) and np.array_equal(q20.rev[:2], want.rev[:2]))
    res["Q20_interior_count_fraction"] = float(q20.fwd[2:].sum() + q20.rev[2:].sum()) / float(want.fwd[2:].sum() + want.rev[2:].sum())
    eng.close()
    eng = engine(min_base_qual=20, length_bins=EDGES[shape])
    res["ms"]["Q20_S_4_edges"] = timed(eng)
    bins = eng.finish_bins()
    res["Q20_bins_sum_to_Q20"] = bool(np.array_equal(sum(t.fwd for t in bins.values()), q20.fwd) and
                                      np.array_equal(sum(t.rev for t in bins.values()), q20.rev))
    eng.close()
    ms = res["ms"]
    res["ratio_Q20_over_R"] = ms["Q20"] / ms["R_keeps_every_record"]
    res["ratio_Q20_over_AUTO"] = ms["Q20"] / ms["unmasked_AUTO"]
    res["ratio_Q20_over_TILED"] = ms["Q20"] / ms["unmasked_TILED"]
    res["ratio_Q20_S4_over_Q20"] = ms["Q20_S_4_edges"] / ms["Q20"]
    res["reads_per_s"] = {k: a.reads / (v * 1e-3) for k, v in ms.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale-genome", type=float, default=0.05)
    ap.add_argument("--shapes", default="C3,C4")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bq_bench.json"))
    a = ap.parse_args()
    pkg = ge.load_pkg()
    from pss_bam_amd import synth
    res = {"reads": a.reads, "repeats": a.repeats, "runs": a.runs, "scale_genome": a.scale_genome,
           "statistic": "best of repeats, tally kernels only (Engine.kernel_time); unmasked legs: best of runs",
           "quals": "seeded random Phred 2..41, every record carries RG:Z:L000", "baseline_only": a.baseline_only,
           "shapes": {}}
    for shape in a.shapes.split(","):
        res["shapes"][shape] = bench_shape(pkg, synth, shape, a)
    if a.parent_json:
        parent = json.loads(Path(a.parent_json).read_text())
        res["parent"] = {"same_session": True, "shapes": {}}
        for shape, mine in res["shapes"].items():
            theirs = parent["shapes"][shape]["unmasked_runs"]
            cmp_ = {}
            for leg, pr in theirs.items():
                here = mine["unmasked_runs"][leg]
                cmp_[leg] = {"parent": pr, "this_commit_median_over_parent_median": here["median_ms"] / pr["median_ms"],
                             "this_commit_min_over_parent_min": here["min_ms"] / pr["min_ms"],
                             # not slower than the parent's own slowest run of the same leg
                             "within_parent_spread": bool(here["median_ms"] <= pr["max_ms"])}
            res["parent"]["shapes"][shape] = cmp_
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

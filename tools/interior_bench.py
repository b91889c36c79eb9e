"""pss-bam -W cost: tally-kernel time of plain <150>M records without the interior table, with the mismatch histogram the
INTERIOR arm shares its walk with (-N 10), with the table at margin 15 and at margin 0, with the table under -Q 20, and with
-Q 20 alone.

    python tools/interior_bench.py [--reads 4000000] [--repeats 5] [--rounds 3] [--scale-genome 1.0] [--region-len 15]
                                   [--out profiles/interior_bench.json]

Rows: plain_tiled (KERNEL_TILED, the kernel the arm is built into), N10 (the MISM arm), W15, W0, W15_Q20 (the INTERIOR arm,
the last one with MASKQ), Q20 (MASKQ alone).  Every row has its own engine over the same records and genome; the rows are
visited in turn, --rounds times, so that drift of the clocks meets all of them alike.  Engine.kernel_time() sums the tally
launches' own durations (HIP events), so copies are not included; a figure is the best of --repeats submits in one visit.
The rows with the table assert reads == pss_ok and that the whole-read table holds more bases than the one at margin 15."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
READ_LEN = 150
ROWS = {"plain_tiled": {}, "N10": dict(mismatches=(10, -1, 0)), "W15": dict(interior=15), "W0": dict(interior=0),
        "W15_Q20": dict(interior=15, min_base_qual=20), "Q20": dict(min_base_qual=20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--region-len", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "interior_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    from pss_bam_amd import synth

    d = synth.config("C2", n_reads=a.reads, scale_genome=a.scale_genome)
    d.pop("region_len")
    d.update(len_min=READ_LEN, len_max=READ_LEN)
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]

    engines = {}
    for row, kw in ROWS.items():
        eng = pkg.Engine(pss=dict(region_len=a.region_len), kernel=pkg.KERNEL_TILED, **kw)
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        engines[row] = eng
    ms = {row: [] for row in ROWS}
    for _ in range(a.rounds):
        for row, eng in engines.items():
            best = None
            eng.kernel_time(reset=True)
            for _ in range(a.repeats):
                eng.submit(recs, offs)
                eng.sync()
                t, _ = eng.kernel_time(reset=True)
                best = t if best is None else min(best, t)
            ms[row].append(best)
    sec = {"reads": a.reads, "read_len": READ_LEN, "region_len": a.region_len, "repeats": a.repeats, "rounds": a.rounds,
           "record_bytes_mean": float(offs[-1]) / a.reads,
           "statistic": "per visit: best of repeats, tally kernels only (Engine.kernel_time); ms lists one figure per round",
           "ms": ms, "best_ms": {row: min(v) for row, v in ms.items()}, "pss_ok": {}, "interior_reads": {}, "interior_bases": {}}
    n_submits = a.rounds * a.repeats
    for row, eng in engines.items():
        if "interior" in ROWS[row]:
            table, reads = eng.finish_interior()
        st = eng.finish().stats
        sec["pss_ok"][row] = st["pss_ok"] // n_submits
        if "interior" in ROWS[row]:
            assert reads == st["pss_ok"] > 0, (row, reads, st["pss_ok"])
            sec["interior_reads"][row], sec["interior_bases"][row] = reads // n_submits, int(table.sum()) // n_submits
        eng.close()
    assert sec["interior_bases"]["W0"] > sec["interior_bases"]["W15"] >= sec["interior_bases"]["W15_Q20"] > 0
    for ref in ("plain_tiled", "N10"):
        sec[f"over_{ref}"] = {row: sec["best_ms"][row] / sec["best_ms"][ref] for row in ROWS}
        sec[f"over_{ref}_spread"] = {row: [min(ms[row]) / max(ms[ref]), max(ms[row]) / min(ms[ref])] for row in ROWS}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()

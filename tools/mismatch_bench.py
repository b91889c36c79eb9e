"""pss-bam -n / -N / -V cost: tally-kernel time of plain <150>M records without the mismatch count, with the filter
(-n 3), with the histogram (-N 10), with both, and with both counting transversions only.

    python tools/mismatch_bench.py [--reads 4000000] [--repeats 5] [--rounds 3] [--scale-genome 1.0] [--region-len 15]
                                   [--out profiles/mismatch_bench.json]

Rows: plain (KERNEL_AUTO: tally_compact at -r <= 16), plain_tiled (KERNEL_TILED, the kernel the MISM arm is built into),
n3, N10, n3_N10, n3_N10_V (KERNEL_AUTO: the MISM arm of tally_tiled).  Every row has its own engine over the same records
and genome; the rows are visited in turn, --rounds times, so that drift of the clocks meets all of them alike.
Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included; a figure is the best
of --repeats submits in one visit.  The rows with a histogram assert sum(mf) == sum(mr) == pss_ok (every record is
unpaired), the rows with a filter that it filtered something and kept something."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
READ_LEN = 150
ROWS = {"plain": None, "plain_tiled": None, "n3": (0, 3, 0), "N10": (10, -1, 0), "n3_N10": (10, 3, 0), "n3_N10_V": (10, 3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--region-len", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mismatch_bench.json"))
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
    for row, mism in ROWS.items():
        eng = pkg.Engine(pss=dict(region_len=a.region_len), kernel=pkg.KERNEL_TILED if row == "plain_tiled" else pkg.KERNEL_AUTO, mismatches=mism)
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
           "ms": ms, "best_ms": {row: min(v) for row, v in ms.items()}, "pss_ok": {}, "pss_filtered": {}, "histogram": {}}
    n_submits = a.rounds * a.repeats
    for row, eng in engines.items():
        mism = ROWS[row]
        if mism and mism[0]:
            mf, mr = eng.finish_mismatches()
        st = eng.finish().stats
        sec["pss_ok"][row], sec["pss_filtered"][row] = st["pss_ok"] // n_submits, st["pss_filtered"] // n_submits
        if mism and mism[0]:
            assert int(mf.sum()) == int(mr.sum()) == st["pss_ok"] > 0, (row, int(mf.sum()), st["pss_ok"])
            sec["histogram"][row] = [int(v) // n_submits for v in mf]
        if mism and mism[1] >= 0:
            assert 0 < st["pss_ok"] and st["pss_filtered"] > engines["plain"].finish().stats["pss_filtered"], row
        eng.close() if row != "plain" else None
    engines["plain"].close()
    sec["over_plain_tiled"] = {row: sec["best_ms"][row] / sec["best_ms"]["plain_tiled"] for row in ROWS}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()

"""pss-bam -P cost: tally-kernel time of plain <150>M records without the composition table, with it at width 10 and at width
30, with width 10 under a region filter, with the region filter alone, and with the interior table (-W 15) as the yardstick of
the previous arm.

    python tools/composition_bench.py [--reads 4000000] [--repeats 5] [--rounds 3] [--scale-genome 1.0] [--region-len 15]
                                      [--out profiles/composition_bench.json]

Rows: plain_tiled (KERNEL_TILED, the kernel the arm is built into), P10, P30 (the COMP arm), P10_T (with REGIONS: the first
half of every contig), T (REGIONS alone), W15 (the INTERIOR arm).  Every row has its own engine over the same records and
genome; the rows are visited in turn, --rounds times, so that drift of the clocks meets all of them alike.
Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included; a figure is the best of
--repeats submits in one visit.  The rows with the table assert that the row next to the read (offset -1) of each block holds
one count per read that was added to that block's table, and that widths 10 and 30 agree on the rows they share."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
READ_LEN = 150
ROWS = {"plain_tiled": {}, "P10": dict(composition=10), "P30": dict(composition=30), "P10_T": dict(composition=10), "T": {},
        "W15": dict(interior=15)}
WITH_REGIONS = ("P10_T", "T")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--region-len", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "composition_bench.json"))
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
    # -T: the first half of every contig
    region_names = [nm for nm, _ in genome]
    regions = (region_names, np.arange(len(genome), dtype=np.int32), np.zeros(len(genome), dtype=np.uint32),
               np.array([len(g) // 2 for _, g in genome], dtype=np.uint32))

    engines = {}
    for row, kw in ROWS.items():
        eng = pkg.Engine(pss=dict(region_len=a.region_len), kernel=pkg.KERNEL_TILED, **kw)
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        if row in WITH_REGIONS:
            eng.set_regions(*regions)
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
           "ms": ms, "best_ms": {row: min(v) for row, v in ms.items()}, "pss_ok": {}, "composition_next_to_read": {}}
    n_submits = a.rounds * a.repeats
    blocks = {}
    for row, eng in engines.items():
        w = ROWS[row].get("composition")
        if w:
            blocks[row] = eng.finish_composition()
        tot = eng.finish()
        st = tot.stats
        sec["pss_ok"][row] = st["pss_ok"] // n_submits
        if w:
            c5, c3 = blocks[row]
            # offset -1 exists for every read that was added: its row is the diagonal of the table's first context row
            assert int(c5[w - 1, :4].sum()) == int(tot.fwd[1].sum()) > 0 and int(c3[w - 1, :4].sum()) == int(tot.rev[1].sum()) > 0, row
            sec["composition_next_to_read"][row] = [int(c5[w - 1].sum()) // n_submits, int(c3[w - 1].sum()) // n_submits]
        eng.close()
    assert np.array_equal(blocks["P10"][0], blocks["P30"][0][20:40]) and np.array_equal(blocks["P10"][1], blocks["P30"][1][20:40])
    assert 0 < sec["pss_ok"]["P10_T"] == sec["pss_ok"]["T"] < sec["pss_ok"]["P10"] == sec["pss_ok"]["plain_tiled"]
    for ref in ("plain_tiled", "W15", "T"):
        sec[f"over_{ref}"] = {row: sec["best_ms"][row] / sec["best_ms"][ref] for row in ROWS}
        sec[f"over_{ref}_spread"] = {row: [min(ms[row]) / max(ms[ref]), max(ms[row]) / min(ms[ref])] for row in ROWS}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()

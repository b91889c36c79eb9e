"""pss-bam -y / -Y cost: tally-kernel time of plain <150>M records without the read score, with the filter (-y 3), with the
histogram (-Y), with both -- and, for scale, with the mismatch filter (-n 3) and the interior table (-W 15) -- each also
under a minimum base quality (-Q 20).

    python tools/read_score_bench.py [--reads 4000000] [--repeats 5] [--rounds 3] [--scale-genome 1.0] [--region-len 15]
                                     [--out profiles/read_score_bench.json]

Rows: plain_tiled (KERNEL_TILED, the kernel the other arms are built into), n3, W15, y3, Y, y3_Y, and the same six with
_Q20.  The weights are the table the command line uses (pss_pmd_weights), the histogram is the command line's (64 rows of
one nat).  Every row has its own engine over the same records and genome; the rows are visited in turn, --rounds times, so
that drift of the clocks meets all of them alike.  Engine.kernel_time() sums the tally launches' own durations (HIP
events), so copies are not included; a figure is the best of --repeats submits in one visit.  Ratios are against
plain_tiled of the same round; the file gives the ratio of the best figures and the smallest and largest ratio of a round.
The rows with a histogram assert sum(sf) == sum(sr) == pss_ok (every record is unpaired), the rows with a filter that it
filtered something (what it kept is recorded as pss_ok)."""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
READ_LEN = 150
BASE_ROWS = ("plain_tiled", "n3", "W15", "y3", "Y", "y3_Y")


def row_settings(row: str, weights) -> dict:
    """the Engine keywords of a row"""
    name, _, q = row.partition("_Q")
    kw = {"min_base_qual": int(q)} if q else {}
    if name == "n3":
        kw["mismatches"] = (0, 3, 0)
    elif name == "W15":
        kw["interior"] = 15
    elif name != "plain_tiled":
        kw["read_score"] = dict(weights=weights, min_score=3 * 256 if "y3" in name else None,
                                hist_half=32 if name.endswith("Y") else 0, hist_shift=8 if name.endswith("Y") else 0)
    return kw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--region-len", type=int, default=15)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "read_score_bench.json"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    from pss_bam_amd import synth

    host = C.CDLL(str(pkg.LIB_HOST))
    weights = np.zeros((4, 32, 64), dtype=np.int16)
    host.pss_pmd_weights.argtypes = [C.c_void_p]
    host.pss_pmd_weights.restype = None
    host.pss_pmd_weights(weights.ctypes.data)

    d = synth.config("C2", n_reads=a.reads, scale_genome=a.scale_genome)
    d.pop("region_len")
    d.update(len_min=READ_LEN, len_max=READ_LEN)
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]

    rows = list(BASE_ROWS) + [f"{r}_Q20" for r in BASE_ROWS]
    engines = {}
    for row in rows:
        eng = pkg.Engine(pss=dict(region_len=a.region_len), kernel=pkg.KERNEL_TILED, **row_settings(row, weights))
        eng.set_genome_arrays(genome)
        eng.set_references(names)
        engines[row] = eng
    ms = {row: [] for row in rows}
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
    stats = {}
    for row, eng in engines.items():
        kw = row_settings(row, weights)
        hist = eng.finish_read_score() if kw.get("read_score", {}).get("hist_half") else None
        st = stats[row] = eng.finish().stats
        sec["pss_ok"][row], sec["pss_filtered"][row] = st["pss_ok"] // n_submits, st["pss_filtered"] // n_submits
        if hist is not None:
            assert int(hist[0].sum()) == int(hist[1].sum()) == st["pss_ok"], (row, int(hist[0].sum()), st["pss_ok"])
            sec["histogram"][row] = [int(v) // n_submits for v in hist[0]]
        if "n3" in row or "y3" in row:
            assert st["pss_filtered"] > stats["plain_tiled"]["pss_filtered"], row   # (what it kept is in pss_ok)
        eng.close()
    per_round = {row: [ms[row][k] / ms["plain_tiled"][k] for k in range(a.rounds)] for row in rows}
    sec["over_plain_tiled"] = {row: {"best": sec["best_ms"][row] / sec["best_ms"]["plain_tiled"], "min": min(per_round[row]), "max": max(per_round[row])}
                               for row in rows}
    sec["plain_tiled_spread_ms"] = [min(ms["plain_tiled"]), max(ms["plain_tiled"])]
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(sec, indent=1) + "\n")
    print(json.dumps(sec))


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()

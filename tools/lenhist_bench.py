"""pss-bam -H cost: tally-kernel time of plain <L>M records with and without the fragment-length histogram, at
-r 15 and -r 25, for the two distributions that matter to its atomics: every read one length (a modern library: all
reads meet in one bin) and lengths spread over 30..150.

    python tools/lenhist_bench.py [--reads 4000000] [--repeats 5] [--runs 3] [--scale-genome 1.0]
                                  [--tree <checkout>] [--label this] [--out profiles/lenhist_bench.json]

Legs per (distribution, -r):  a = no histogram, KERNEL_AUTO;  b = no histogram, KERNEL_TILED;  h = histogram with
limit 300 (KERNEL_AUTO: the HIST arm of tally_tiled).  "c" of the issue is h on one_length, "d" is h on spread.
Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included; a figure is
the best of --repeats submits, and every leg is measured --runs times to show the run-to-run spread.  The histogram
legs assert sum(hf) == sum(hr) == pss_ok (every record is unpaired).

--tree times another checkout of the project with this script (the parent commit, built there), --label names the
section of the output file the figures go to; a tree without the histogram runs legs a and b only.  With both "this"
and "parent" in the file the ratios h / b_parent are added."""
import argparse
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
HIST_MAX = 300
DISTRIBUTIONS = {"one_length": (100, 100), "spread_30_150": (30, 150)}
REGION_LENS = (15, 25)


def load_tree(tree: Path):
    spec = importlib.util.spec_from_file_location("graft_entry_of_tree", tree / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_pkg()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--tree", default=str(ROOT))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lenhist_bench.json"))
    a = ap.parse_args()
    pkg = load_tree(Path(a.tree).resolve())
    from pss_bam_amd import synth
    has_hist = hasattr(pkg.Engine, "set_length_histogram")

    sec = {"reads": a.reads, "repeats": a.repeats, "runs": a.runs, "hist_max": HIST_MAX if has_hist else None,
           "statistic": "per run: best of repeats, tally kernels only (Engine.kernel_time); ms lists one figure per run",
           "record_bytes_mean": {}, "ms": {}, "hist_sums_to_pss_ok": {}}
    for dist, (lo, hi) in DISTRIBUTIONS.items():
        d = synth.config("C2", n_reads=a.reads, scale_genome=a.scale_genome)
        d.pop("region_len")
        d.update(len_min=lo, len_max=hi)
        scfg = synth.make_cfg(**d)
        recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
        last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
        names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
        genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]
        sec["record_bytes_mean"][dist] = float(offs[-1]) / a.reads

        def timed(eng) -> list:
            out = []
            for _ in range(a.runs):
                best = None
                eng.kernel_time(reset=True)
                for _ in range(a.repeats):
                    eng.submit(recs, offs)
                    eng.sync()
                    ms, _ = eng.kernel_time(reset=True)
                    best = ms if best is None else min(best, ms)
                out.append(best)
            return out

        for n in REGION_LENS:
            legs = [("a", pkg.KERNEL_AUTO, {}), ("b", pkg.KERNEL_TILED, {})]
            if has_hist:
                legs.append(("h", pkg.KERNEL_AUTO, {"length_hist": HIST_MAX}))
            for leg, kernel, kw in legs:
                eng = pkg.Engine(pss=dict(region_len=n), kernel=kernel, **kw)
                eng.set_genome_arrays(genome)
                eng.set_references(names)
                key = f"{dist}/r{n}/{leg}"
                sec["ms"][key] = timed(eng)
                if kw:
                    hf, hr = eng.finish_length_hist()
                    ok = eng.finish().stats["pss_ok"]
                    assert int(hf.sum()) == int(hr.sum()) == ok and ok > 0.9 * a.runs * a.repeats * a.reads, (key, int(hf.sum()), ok)
                    assert np.count_nonzero(hf) == 1 if lo == hi else np.count_nonzero(hf) > (hi - lo) // 2, key
                    sec["hist_sums_to_pss_ok"][key] = True
                eng.close()
        del recs, offs, genome

    out = Path(a.out)
    res = json.loads(out.read_text()) if out.exists() else {}
    res[a.label] = sec
    if "this" in res and "parent" in res:
        # the yardstick: legs a and b of this commit against the parent's runs, the histogram legs against the parent's b
        cmp = {}
        for key, runs in res["this"]["ms"].items():
            base, leg = key.rsplit("/", 1)
            pb = res["parent"]["ms"].get(f"{base}/b")
            pa = res["parent"]["ms"].get(key)
            if leg == "h" and pb:
                cmp[f"{base}/h_over_b_parent"] = min(runs) / min(pb)
            elif pa:
                cmp[f"{key}_over_parent"] = min(runs) / min(pa)
                cmp[f"{key}_parent_spread"] = max(pa) / min(pa)
        res["ratios_best_run"] = cmp
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({a.label: sec, "ratios_best_run": res.get("ratios_best_run")}))


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()

"""pss-bam -E cost: tally-kernel time of plain <L>M records with and without the end condition, at -r 15 and -r 25.

    python tools/end_condition_bench.py [--reads 4000000] [--repeats 5] [--runs 3] [--scale-genome 1.0]
                                        [--tree <checkout>] [--label this] [--out profiles/end_condition_bench.json]

Legs per -r:  b = no end condition, KERNEL_TILED (the parent's leg when the tree is the parent commit's, this commit
without -E when it is this one's);  e1 = -E ss (depth 1, cells TC / TC), e8 = -E ss,8 (KERNEL_AUTO: the END arm of
tally_tiled).
Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included; a figure is
the best of --repeats submits, and every leg is measured --runs times to show the run-to-run spread.  The e legs
assert that COND stays below T and record the input's marked fractions reads[1..3] / reads[0]: the second LDS add
scales with them.

--tree times another checkout of the project with this script (the parent commit, built there), --label names the
section of the output file the figures go to; a tree without the setter runs leg b only.  With both "this" and
"parent" in the file the ratios b / b_parent (beside the parent's own run-to-run spread) and e / b_parent are added."""
import argparse
import importlib.util
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
REGION_LENS = (15, 25)
LEN_RANGE = (30, 150)


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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "end_condition_bench.json"))
    a = ap.parse_args()
    pkg = load_tree(Path(a.tree).resolve())
    from pss_bam_amd import synth
    has_end = hasattr(pkg.Engine, "set_end_condition")

    d = synth.config("C2", n_reads=a.reads, scale_genome=a.scale_genome)
    d.pop("region_len")
    d.update(len_min=LEN_RANGE[0], len_max=LEN_RANGE[1])
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]
    sec = {"reads": a.reads, "repeats": a.repeats, "runs": a.runs, "read_lengths": list(LEN_RANGE),
           "statistic": "per run: best of repeats, tally kernels only (Engine.kernel_time); ms lists one figure per run",
           "record_bytes_mean": float(offs[-1]) / a.reads, "ms": {}, "marked_fraction_5p_3p_both": {}}

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
        legs = [("b", pkg.KERNEL_TILED, {})]
        if has_end:
            legs += [("e1", pkg.KERNEL_AUTO, {"end_condition": (1, 13, 13)}), ("e8", pkg.KERNEL_AUTO, {"end_condition": (8, 13, 13)})]
        for leg, kernel, kw in legs:
            eng = pkg.Engine(pss=dict(region_len=n), kernel=kernel, **kw)
            eng.set_genome_arrays(genome)
            eng.set_references(names)
            key = f"r{n}/{leg}"
            sec["ms"][key] = timed(eng)
            if kw:
                cf, cr, reads = eng.finish_end_condition()
                tot = eng.finish()
                assert tot.stats["pss_ok"] > 0.9 * a.runs * a.repeats * a.reads, key
                assert reads[0] > 0 and (cf <= tot.fwd).all() and (cr <= tot.rev).all() and int(cf[0].sum()) <= int(reads[2]), key
                sec["marked_fraction_5p_3p_both"][key] = [float(reads[k]) / float(reads[0]) for k in (1, 2, 3)]
            eng.close()

    out = Path(a.out)
    res = json.loads(out.read_text()) if out.exists() else {}
    res[a.label] = sec
    if "this" in res and "parent" in res:
        cmp = {}
        for key, runs in res["this"]["ms"].items():
            base, leg = key.rsplit("/", 1)
            pb = res["parent"]["ms"].get(f"{base}/b")
            if not pb:
                continue
            cmp[f"{key}_over_b_parent"] = min(runs) / min(pb)
            cmp[f"{base}/b_parent_spread"] = max(pb) / min(pb)
        res["ratios_best_run"] = cmp
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({a.label: sec, "ratios_best_run": res.get("ratios_best_run")}))


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()

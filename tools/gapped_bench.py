"""pss-bam -I cost: tally-kernel time of C4-shaped synthetic records (cigar_mix = 1: 30 % of them carry S / I / D variants)
with and without the anchored-ends tally, at -r 15 and -r 25, against the parent commit measured in the same session.

    python tools/gapped_bench.py --parent-tree <checkout of the parent commit, built> [--reads 4000000] [--repeats 5]
                                 [--runs 3] [--scale-genome 1.0] [--out profiles/gapped_bench.json]

Legs per -r:  p = the parent tree, KERNEL_TILED;  b = this tree, KERNEL_TILED without -I (the same instantiations);
g = this tree, KERNEL_TILED with gapped=True.  A run is a fresh child process that builds the records and the genome
(the generator is deterministic: every child times the same bytes) and times every leg of ONE tree; the runs of the
two trees alternate (parent, this, parent, this, ...), --runs of each.  Engine.kernel_time() sums the tally launches'
own durations (HIP events), so copies are not included; a figure is the best of --repeats submits.

Written: the per-run figures, b / p of the best runs beside the parent's own run-to-run spread (b has to lie inside
it), g / p, and the share of records that -I adds to the tables (pss_ok with over pss_ok without)."""
import argparse
import importlib.util
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
REGION_LENS = (15, 25)


def load_tree(tree: Path):
    spec = importlib.util.spec_from_file_location("graft_entry_of_tree", tree / "__graft_entry__.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.load_pkg()


def one_run(a) -> dict:
    """every leg of the tree a.tree once; -> {"ms": {leg key: best of repeats}, "pss_ok": {leg key: per submit}}"""
    pkg = load_tree(Path(a.tree).resolve())
    from pss_bam_amd import synth
    d = synth.config("C4", n_reads=a.reads, scale_genome=a.scale_genome)
    d.pop("region_len")
    assert d["cigar_mix"]
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    names = [synth.contig_name(scfg, k) for k in range(int(scfg.n_contigs))]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]
    has_gapped = hasattr(pkg.Engine, "set_gapped")
    out = {"ms": {}, "pss_ok": {}, "slow_path": {}, "record_bytes_mean": float(offs[-1]) / a.reads}
    for n in REGION_LENS:
        legs = [("p" if a.label == "parent" else "b", {})]
        if has_gapped and a.label != "parent":
            legs.append(("g", {"gapped": True}))
        for leg, kw in legs:
            eng = pkg.Engine(pss=dict(region_len=n), kernel=pkg.KERNEL_TILED, **kw)
            eng.set_genome_arrays(genome)
            eng.set_references(names)
            best = None
            eng.kernel_time(reset=True)
            for _ in range(a.repeats):
                eng.submit(recs, offs)
                eng.sync()
                ms, _ = eng.kernel_time(reset=True)
                best = ms if best is None else min(best, ms)
            st = eng.finish().stats
            eng.close()
            key = f"r{n}/{leg}"
            out["ms"][key] = best
            out["pss_ok"][key] = st["pss_ok"] / a.repeats
            out["slow_path"][key] = st["slow_path"] / a.repeats
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "gapped_bench.json"))
    ap.add_argument("--tree", help="(a child run: the tree to time)")
    ap.add_argument("--label", help="(a child run: parent or this)")
    a = ap.parse_args()
    if a.tree:
        print("RESULT " + json.dumps(one_run(a)))
        return
    if not a.parent_tree:
        ap.error("--parent-tree is required: the parent commit is timed in the same session")
    trees = {"parent": Path(a.parent_tree).resolve(), "this": ROOT}
    runs = {"parent": [], "this": []}
    for _ in range(a.runs):
        for label in ("parent", "this"):       # alternating; a fresh process each, so neither tree inherits the other's loaded library
            pr = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--tree", str(trees[label]), "--label", label, "--reads", str(a.reads),
                                 "--repeats", str(a.repeats), "--scale-genome", str(a.scale_genome)], capture_output=True, text=True, timeout=900)
            if pr.returncode != 0:
                sys.exit(f"{label} run failed ({pr.returncode}):\n{pr.stderr[-3000:]}")
            runs[label].append(json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    res = {"reads": a.reads, "repeats": a.repeats, "runs": a.runs, "workload": "synth C4 (cigar_mix = 1, 30-80 bp)",
           "statistic": "per run: best of repeats, tally kernels only (Engine.kernel_time); ms lists one figure per run, runs of the two trees alternating",
           "record_bytes_mean": runs["this"][0]["record_bytes_mean"], "ms": {}, "ratios_best_run": {}}
    for label in runs:
        for key in runs[label][0]["ms"]:
            res["ms"][key] = [r["ms"][key] for r in runs[label]]
    for n in REGION_LENS:
        p, b, g = (res["ms"][f"r{n}/{leg}"] for leg in "pbg")
        ok_b, ok_g = runs["this"][0]["pss_ok"][f"r{n}/b"], runs["this"][0]["pss_ok"][f"r{n}/g"]
        res["ratios_best_run"][f"r{n}"] = {"p_spread": max(p) / min(p), "b_over_p": min(b) / min(p), "b_inside_p_spread": min(p) <= min(b) <= max(p) or min(b) <= min(p),
                                           "g_over_p": min(g) / min(p), "reads_tallied_without": ok_b, "reads_tallied_with": ok_g,
                                           "share_of_records_added": (ok_g - ok_b) / a.reads, "one_lane_path_records_with": runs["this"][0]["slow_path"][f"r{n}/g"]}
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    main()

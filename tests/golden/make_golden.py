#!/usr/bin/env python3
"""Regenerates tests/golden/* by running the UNMODIFIED reference (oracle/_ref, built by
oracle/Makefile from the reference sources) on small synthetic inputs made by
tests/pssbam_testlib.py.  Only data is written here: inputs (FASTA, SAM, and the BAM
encoding of the same records) and the reference's outputs for them; for the larger fuzz
sets of test_oracle_vs_ref.py only the outputs (fuzz_ref.npz: report texts, sparse k-mer
tables, and a digest of the inputs each was made from), since the tests regenerate those
inputs from their seeds.

    python tests/golden/make_golden.py        # needs oracle/_ref (i.e. the reference sources)

The committed fixtures were produced by exactly this script.
"""
import json
import sys
from dataclasses import asdict
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import pssbam_testlib as tl  # noqa: E402
from pssbam_testlib import (FkOpts, PssOpts, build_oracle, fuzz_dataset, have_ref, ref_safe,  # noqa: E402
                            run_ref_fragkon, run_ref_gkc, run_ref_pss, write_bam, write_fasta, write_sam)
import numpy as np  # noqa: E402


def fuzz_vectors(work: Path) -> dict:
    """the reference's outputs on the fuzz sets of test_oracle_vs_ref.py, generated in `work`"""
    import os
    out = {}
    text = lambda s: np.frombuffer(s.encode(), dtype=np.uint8)  # noqa: E731
    cwd = os.getcwd()
    try:
        for seed in range(tl.FUZZ_SEEDS):
            d = work / f"pss{seed}"
            d.mkdir()
            os.chdir(d)
            fa, sam, opts = tl.pss_fuzz_case(seed)
            for trial, o in enumerate(opts):
                key = f"pss_{seed}_{trial}"
                _, _, ct, rt, _ = run_ref_pss(Path(fa), Path(sam), Path(f"ref{trial}"), o)
                out[key + "_counts"], out[key + "_rates"] = text(ct), text(rt)
                out[key + "_inputs"] = np.array(tl.inputs_digest([fa, sam], o))
        for seed in range(tl.FUZZ_SEEDS):
            d = work / f"fk{seed}"
            d.mkdir()
            os.chdir(d)
            fa, trials = tl.fk_fuzz_case(seed)
            for trial, (o, sam) in enumerate(trials):
                key = f"fk_{seed}_{trial}"
                k5, k3, _, _ = run_ref_fragkon(Path(fa), Path(sam), o)
                out[key + "_idx"], out[key + "_k5"], out[key + "_k3"] = tl.sparse(k5, k3)
                out[key + "_inputs"] = np.array(tl.inputs_digest([fa, sam], o))
        d = work / "gz"
        d.mkdir()
        os.chdir(d)
        fa, fagz, sam, o = tl.gz_fuzz_case()
        out["gz_counts"] = text(run_ref_pss(Path(fa), Path(sam), Path("p0"), o)[2])
        out["gz_counts_O2"] = text(run_ref_pss(Path(fagz), Path(sam), Path("p1"), o, variant="pss-bam.O2")[2])
        out["gz_inputs"] = np.array(tl.inputs_digest([fa, sam], o))
        for k in tl.GKC_KS:
            d = work / f"gkc{k}"
            d.mkdir()
            os.chdir(d)
            fa = tl.gkc_fuzz_case(k)
            out[f"gkc_{k}_idx"], out[f"gkc_{k}_counts"] = tl.sparse(run_ref_gkc(Path(fa), k)[0])
            out[f"gkc_{k}_inputs"] = np.array(tl.inputs_digest([fa]))
    finally:
        os.chdir(cwd)
    return out


def main():
    build_oracle()
    assert have_ref(), "oracle/_ref missing: this script needs the reference sources"
    manifest = {"note": "expected outputs produced by oracle/_ref (unmodified reference); see make_golden.py",
                "datasets": {}, "cases": []}

    # dataset A: branch-coverage fuzz set, no aux tags; dataset B: with RG / NM / XA tags
    for name, seed, n, with_rg in (("A", 424242, 700, False), ("B", 515151, 500, True)):
        contigs, refs, recs = fuzz_dataset(seed, n, with_rg=with_rg)
        recs = ref_safe(recs, klen=5)   # keeps the set valid for every k <= 5 case below
        fa = HERE / f"set{name}.fa"
        sam = HERE / f"set{name}.sam"
        bam = HERE / f"set{name}.bam"
        write_fasta(fa, contigs, width=60)
        write_sam(sam, refs, recs)
        write_bam(bam, refs, recs, level=6, rng=np.random.default_rng(seed))
        manifest["datasets"][name] = {"fasta": fa.name, "sam": sam.name, "bam": bam.name, "n_records": len(recs)}

    pss_cases = [
        ("A", PssOpts()),
        ("A", PssOpts(region_len=25, min_mq=20)),
        ("A", PssOpts(region_len=8, min_read_len=20, max_read_len=70, up_ctx="CT", down_ctx="AG", merged_only=True)),
        ("A", PssOpts(region_len=40, up_ctx="ACGTN")),
        ("B", PssOpts(region_len=10)),
        ("B", PssOpts(region_len=10, read_group="grpA")),
        ("B", PssOpts(region_len=15, read_group="grpB", min_mq=10)),
    ]
    for i, (ds, o) in enumerate(pss_cases):
        d = manifest["datasets"][ds]
        tag = f"pss_{i}"
        # -F/-B/-o strings are echoed into the report headers: run with cwd-relative names
        import os
        cwd = os.getcwd()
        os.chdir(HERE)
        try:
            run_ref_pss(Path(d["fasta"]), Path(d["sam"]), Path(tag), o)
        finally:
            os.chdir(cwd)
        manifest["cases"].append({"tool": "pss-bam", "dataset": ds, "opts": asdict(o), "prefix": tag,
                                  "counts": f"{tag}.pss.counts.txt", "rates": f"{tag}.pss.rates.txt"})

    fk_cases = [("A", FkOpts(klen=4)), ("A", FkOpts(klen=3, min_mq=20)), ("A", FkOpts(klen=5, merged_only=True)),
                ("A", FkOpts(klen=2, min_read_len=30, max_read_len=80)), ("B", FkOpts(klen=1))]
    for i, (ds, o) in enumerate(fk_cases):
        d = manifest["datasets"][ds]
        tag = f"fragkon_{i}.txt"
        import os
        cwd = os.getcwd()
        os.chdir(HERE)
        try:
            _, _, out, _ = run_ref_fragkon(Path(d["fasta"]), Path(d["sam"]), o)
        finally:
            os.chdir(cwd)
        (HERE / tag).write_text(out)
        manifest["cases"].append({"tool": "fragkon", "dataset": ds, "opts": asdict(o), "stdout": tag})

    for ds, k in (("A", 4), ("A", 3), ("B", 6)):
        d = manifest["datasets"][ds]
        tag = f"gkc_{ds}_{k}.txt"
        import os
        cwd = os.getcwd()
        os.chdir(HERE)
        try:
            _, out = run_ref_gkc(Path(d["fasta"]), k)
        finally:
            os.chdir(cwd)
        (HERE / tag).write_text(out)
        manifest["cases"].append({"tool": "genome-kmer-count", "dataset": ds, "klen": k, "stdout": tag})

    (HERE / "manifest.json").write_text(json.dumps(manifest, indent=1) + "\n")
    print(f"wrote {len(manifest['cases'])} golden cases to {HERE}")

    import tempfile
    with tempfile.TemporaryDirectory(prefix="pssbam_golden_") as work:
        vec = fuzz_vectors(Path(work))
    np.savez_compressed(tl.FUZZ_REF, **vec)
    print(f"wrote {len(vec)} fuzz-set arrays to {tl.FUZZ_REF}")


if __name__ == "__main__":
    main()

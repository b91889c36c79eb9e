"""pss-bam -G cost: tally-kernel time of C3-shaped records (150 bp, N = 25) with an RG:Z field appended, for
no filter, -R (one group), and -G with n = 1, 4, 8 and 40 groups (groups dealt by record slot).

    python tools/rg_bench.py [--reads 4000000] [--repeats 5] [--scale-genome 1.0] [--out profiles/rg_bench.json]

Engine.kernel_time() sums the tally launches' own durations (HIP events), so copies are not included.
-R and -G n = 4 run on the same records (4 groups), which is where the target "-G n=4 <= 2x one -R run"
is judged."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import __graft_entry__ as ge  # noqa: E402

ID_LEN = 4   # every ID is 4 bytes ("L000".."L039"): each record grows by the same 3 + 4 + 1 bytes


def with_rg(recs: np.ndarray, offs: np.ndarray, chunk: int = 1 << 18):
    """appends RG:Z:L000 to every record (block_size rewritten) -> (records, offsets, value offsets)"""
    n = offs.size - 1
    grow = 3 + ID_LEN + 1
    new_offs = offs.astype(np.uint64) + grow * np.arange(n + 1, dtype=np.uint64)
    out = np.empty(int(new_offs[-1]), dtype=np.uint8)
    sizes = np.diff(offs.astype(np.int64))
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        src = recs[int(offs[a]):int(offs[b])]
        rec_of_byte = np.repeat(np.arange(a, b, dtype=np.int64), sizes[a:b])
        dst = np.arange(src.size, dtype=np.int64) + int(new_offs[a]) + grow * (rec_of_byte - a)
        out[dst] = src
    tail = new_offs[1:].astype(np.int64) - grow
    for k, byte in enumerate(b"RGZ"):
        out[tail + k] = byte
    out[tail + 3 + ID_LEN] = 0
    bs = np.zeros(n, dtype=np.uint32)
    head = new_offs[:-1].astype(np.int64)
    for k in range(4):
        bs |= out[head + k].astype(np.uint32) << (8 * k)
    bs += grow
    for k in range(4):
        out[head + k] = (bs >> (8 * k)) & 0xFF
    return out, new_offs.astype(np.uint32), tail + 3


def assign(out: np.ndarray, val_at: np.ndarray, n_groups: int) -> list[str]:
    ids = [f"L{k:03d}" for k in range(n_groups)]
    g = np.arange(val_at.size) % n_groups
    codes = np.frombuffer(b"".join(i.encode() for i in ids), dtype=np.uint8).reshape(n_groups, ID_LEN)
    for k in range(ID_LEN):
        out[val_at + k] = codes[g, k]
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scale-genome", type=float, default=1.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rg_bench.json"))
    a = ap.parse_args()
    pkg = ge.load_pkg()
    from pss_bam_amd import synth
    d = synth.config("C3", n_reads=a.reads, scale_genome=a.scale_genome)
    region_len = d.pop("region_len")
    scfg = synth.make_cfg(**d)
    recs, offs = synth.records_host(scfg, 0, a.reads, threads=16)
    last_contig = int(np.frombuffer(recs[int(offs[-2]) + 4:int(offs[-2]) + 8].tobytes(), dtype="<i4")[0])
    n_contigs = int(scfg.n_contigs)
    names = [synth.contig_name(scfg, k) for k in range(n_contigs)]
    genome = [(names[k], synth.genome_host(scfg, k, threads=16)) for k in range(max(last_contig + 1, 1))]
    rg_recs, rg_offs, val_at = with_rg(recs, offs)
    del recs

    def timed(eng) -> float:
        best = None
        eng.kernel_time(reset=True)
        for _ in range(a.repeats):
            eng.submit(rg_recs, rg_offs)
            eng.sync()
            ms, _ = eng.kernel_time(reset=True)
            best = ms if best is None else min(best, ms)
        return best

    res = {"reads": a.reads, "region_len": region_len, "record_bytes_mean": float(rg_offs[-1]) / a.reads,
           "repeats": a.repeats, "statistic": "best of repeats, tally kernels only (Engine.kernel_time)", "ms": {}}
    plain = pkg.Engine(pss=dict(region_len=region_len))
    plain.set_genome_arrays(genome)
    plain.set_references(names)
    assign(rg_recs, val_at, 4)
    res["ms"]["no_filter"] = timed(plain)
    filt = pkg.Engine(pss=dict(region_len=region_len), read_group="L000")
    filt.set_genome_arrays(genome)
    filt.set_references(names)
    res["ms"]["R_one_group_of_4"] = timed(filt)
    filt.close()
    for n in (1, 4, 8, 40):
        ids = assign(rg_recs, val_at, n)
        plain.reset()
        plain.set_read_groups(ids)
        res["ms"][f"G_{n}"] = timed(plain)
        got = plain.finish_groups()
        res.setdefault("unassigned_empty", {})[f"G_{n}"] = int(got[None].fwd.sum() + got[None].rev.sum()) == 0
    plain.close()
    res["ratio_G4_over_R"] = res["ms"]["G_4"] / res["ms"]["R_one_group_of_4"]
    res["target_G4_le_2x_R"] = res["ratio_G4_over_R"] <= 2.0
    res["reads_per_s"] = {k: a.reads / (v * 1e-3) for k, v in res["ms"].items()}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

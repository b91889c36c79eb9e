"""tally_tiled's record staging (LDS-DMA of each record's first pieces, nontemporal policy) against
the oracle at the launch shapes that change what the DMA issues: a last tile shorter than the
others, pieces that would start past the end of the block, a single workgroup that walks every
tile, a grid that is not a multiple of the 8 XCDs, a short tile with records that overflow into
the out-of-line path, and every instantiation of the kernel body (k-mers fused in or not, the
later-row passes of N > 30, -R, -G).  Bit-exact (integer work)."""
import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl
from test_gpu_read_groups import check_engine, oracle_by_group, pss_dict, rg_dataset

pytestmark = pytest.mark.gpu

# environment of the engine -> launch shape of tally_tiled
SHAPES = {
    "default": {},
    "one_workgroup": {"PSSBAM_GRID_WGS": "1"},
    "seven_workgroups": {"PSSBAM_GRID_WGS": "7"},
    "short_tile_overflow": {"PSSBAM_TILE_READS": "64", "PSSBAM_PIECES": "5"},
    "tile_48": {"PSSBAM_TILE_READS": "48"},
}
N_READS = 2001   # not a multiple of any tile size


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


@pytest.fixture(scope="module")
def data():
    return tl.fuzz_dataset(4242, N_READS)


def fk_dict(o: tl.FkOpts) -> dict:
    return dict(klen=o.klen, min_mq=o.min_mq, min_read_len=o.min_read_len, max_read_len=o.max_read_len,
                merged_only=o.merged_only)


def _tiled(pkg, contigs, refs, raw, pss, kmer=None, rg=None):
    eng = pkg.Engine(pss=pss, kmer=kmer, read_group=rg, kernel=pkg.KERNEL_TILED)
    try:
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([n for n, _ in refs])
        eng.submit(raw)
        return eng.finish()
    finally:
        eng.close()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("region_len,klen", [(25, None), (31, None), (62, None), (25, 4), (25, 9), (62, 4)])
def test_tiled_stage_shapes(pkg, oracle, data, tmp_path, monkeypatch, shape, region_len, klen):
    """N = 31 and 62 add the later-row passes; k = 4 tallies k-mers in LDS, k = 9 with global atomics"""
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    contigs, refs, recs = data
    fa, sam = tmp_path / "g.fa", tmp_path / "a.sam"
    tl.write_fasta(fa, contigs)
    tl.write_sam(sam, refs, recs)
    po = tl.PssOpts(region_len=region_len)
    g = oracle.load_genome(fa)
    try:
        wf, wr, st = oracle.pss(g, sam, po)
        fk = None
        if klen is not None:
            ko = tl.FkOpts(klen=klen)
            w5, w3, _ = oracle.fragkon(g, sam, ko)
            fk = fk_dict(ko)
    finally:
        oracle.free_genome(g)
    got = _tiled(pkg, contigs, refs, tl.raw_records(refs, recs), pss_dict(po), kmer=fk)
    assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr)
    assert got.stats["pss_ok"] == st[tl.ST_OK] and got.stats["pss_filtered"] == st[tl.ST_FILTERED]
    if klen is not None:
        assert np.array_equal(got.k5, w5.astype(np.uint64)) and np.array_equal(got.k3, w3.astype(np.uint64))


@pytest.mark.parametrize("shape", ["default", "one_workgroup", "short_tile_overflow"])
def test_tiled_stage_read_group_filter(pkg, oracle, tmp_path, monkeypatch, shape):
    """-R stages whole records (the filter walks the aux fields behind QUAL)"""
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    contigs, refs, recs = tl.fuzz_dataset(4243, N_READS, with_rg=True)
    fa, sam = tmp_path / "g.fa", tmp_path / "a.sam"
    tl.write_fasta(fa, contigs)
    keep = [r for r in recs if ("RG", "Z", "grpA") in r.tags]
    tl.write_sam(sam, refs, keep)
    po = tl.PssOpts(region_len=25)
    g = oracle.load_genome(fa)
    try:
        wf, wr, st = oracle.pss(g, sam, po)
    finally:
        oracle.free_genome(g)
    got = _tiled(pkg, contigs, refs, tl.raw_records(refs, recs), pss_dict(po), rg="grpA")
    assert np.array_equal(got.fwd, wf) and np.array_equal(got.rev, wr)
    assert got.stats["rg_dropped"] == len(recs) - len(keep)


@pytest.mark.parametrize("shape", ["default", "one_workgroup", "seven_workgroups", "short_tile_overflow"])
@pytest.mark.parametrize("region_len", [25, 62])
def test_tiled_stage_groups(pkg, oracle, tmp_path, monkeypatch, shape, region_len):
    """-G with 4 groups (tally_tiled_planes<PLANES_RG>, first and later-row passes)"""
    for k, v in SHAPES[shape].items():
        monkeypatch.setenv(k, v)
    ids = ["lib1", "lib2", "lib3", "lib4"]
    contigs, refs, recs = rg_dataset(4244, ids, n_reads=N_READS)
    raw = tl.raw_records(refs, recs)
    po = tl.PssOpts(region_len=region_len)
    g = oracle.genome_from_arrays(tl.loaded_contigs(contigs))
    try:
        want = oracle_by_group(oracle, g, refs, recs, ids, po, tmp_path)
    finally:
        oracle.free_genome(g)
    eng = pkg.Engine(pss=pss_dict(po), kernel=pkg.KERNEL_TILED, read_groups=ids)
    try:
        eng.set_genome_arrays(tl.loaded_contigs(contigs))
        eng.set_references([n for n, _ in refs])
        eng.submit(raw)
        check_engine(eng, want, ids)
    finally:
        eng.close()

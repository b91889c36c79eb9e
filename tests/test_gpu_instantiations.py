"""Every instantiation of the tiled tally kernels against the oracle.

tally_tiled (68 instantiations, the four of the SCORE arm run by test_gpu_read_score.py), tally_tiled_planes (40),
tally_tiled_kmer_planes (12) and tally_compact (6) are one
kernel per combination of compile-time flags, each with its own register allocation.  The feature tests run every flag;
this module runs every combination: instantiation_lib's configuration list covers the whole census
(test_instantiations_host.py shows that without a GPU, and that no comparison below is vacuous), and each configuration
runs in two launch shapes of test_gpu_tile_loop -- several tiles per workgroup, and the same with five staged pieces so
that every tile also sends records down the one-lane path.  A case is one engine and one launch under KERNEL_AUTO
(every -r is at least 25 or the configuration carries an option, so the tiled family runs); every table the
configuration exposes and the status counters are compared bit for bit (integer work).  The one compact form no other
module launches, PLAN_ONCE with global k-mer bins, runs under the compact shapes like its siblings."""
import pytest

import __graft_entry__ as ge
import instantiation_lib as inl
from test_gpu_tile_loop import NO_XCD, tiled_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


@pytest.fixture(scope="module")
def built(oracle, tmp_path_factory):
    D, A = inl.build_arms(oracle, tmp_path_factory.mktemp("instantiations"))
    assert set(inl.TILED_CONFIGS + inl.COMPACT_CONFIGS) == set(A)
    return D, A


@pytest.mark.parametrize("shape", ["three_wg", "two_wg_overflow"])
@pytest.mark.parametrize("name", inl.TILED_CONFIGS)
def test_tiled_instantiations(pkg, built, monkeypatch, name, shape):
    """tally_tiled, tally_tiled_planes and tally_tiled_kmer_planes: the pass-0 kernel and, at -r 40, the later-pass kernel
    of the same MASKQ / REGIONS (tiled_case asserts slow_path >= 50 under `two_wg_overflow`)"""
    tiled_case(pkg, built, monkeypatch, name, shape)


@pytest.mark.parametrize("shape", NO_XCD)
@pytest.mark.parametrize("name", inl.COMPACT_CONFIGS)
def test_compact_plan_once_with_global_kmer_bins(pkg, built, monkeypatch, name, shape):
    """tally_compact<DO_KMER, !LDS_KMER, PLAN_ONCE>: -r 15 with k = 9 and the plan made once"""
    assert inl.launched(inl.BY_NAME[name]) == {("tally_compact", (1, 0, 1))}
    tiled_case(pkg, built, monkeypatch, name, shape)

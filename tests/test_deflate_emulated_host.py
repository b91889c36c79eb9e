"""The device deflate's encoder without a device: csrc/deflate_kernels.h compiled for the host (tools/deflate_emulate.cpp; a
phase of the workgroup becomes a loop over its threads) under AddressSanitizer + UBSan as a stand-alone program, on the inputs of
tests/test_gpu_deflate.py.  The judges are the same: deflate_lib.walk (Python's zlib) and the fixed cut."""
import gzip
import subprocess
from pathlib import Path

import numpy as np
import pytest

import deflate_lib as dl

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
P = dl.PAYLOAD


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("deflate_emulate") / "deflate_emulate"
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", str(ROOT / "pss-bam_amd" / "csrc"),
                    "-o", str(out), str(ROOT / "tools" / "deflate_emulate.cpp")], check=True, timeout=300)
    return out


def rnd(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def inputs() -> dict:
    a40, a32 = rnd(40000, 2), rnd(32768, 3)
    order = np.random.default_rng(4).permutation(256).astype(np.uint8).tobytes()
    return {
        "one": b"A", "two": b"AB", "three": b"AAA", "four_equal": b"AAAA",
        "equal": b"\x07" * P,
        "random": rnd(P, 1),
        "beyond_the_window": a40 + a40[:P - 40000],
        "at_the_windows_edge": a32 + a32[:P - 32768],
        "256_twice_x3": (bytes(range(256)) + order) * 3,
        "one_literal": b"Q" * 300,
        "fibonacci": dl.fibonacci_payload(),
        "setA": gzip.decompress((GOLD / "setA.bam").read_bytes()),
        "setA_cut_plus_1": gzip.decompress((GOLD / "setA.bam").read_bytes())[:P + 1],
        "setD": gzip.decompress((GOLD / "setD.bam").read_bytes()),
    }


@pytest.mark.parametrize("name", list(inputs()))
def test_emulated_encoder(exe, tmp_path, name):
    raw = inputs()[name]
    (tmp_path / "in.raw").write_bytes(raw)
    pr = subprocess.run([str(exe), str(tmp_path / "in.raw"), str(tmp_path / "out.bgzf")], capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr[-3000:]
    data = (tmp_path / "out.bgzf").read_bytes()
    blocks = dl.check_fixed_cut(data, raw)
    if name == "equal":
        assert dl.btype(blocks[0][0]) == 2 and len(data) < P // 16
    if name == "random":
        assert dl.btype(blocks[0][0]) == 0 and len(data) == P + dl.STORED_EXTRA
    if name == "fibonacci":
        assert dl.huffman_depth(np.bincount(np.frombuffer(raw, dtype=np.uint8))) == 21 and dl.btype(blocks[0][0]) == 2
    if name.startswith("set"):
        assert len(data) < len(raw)

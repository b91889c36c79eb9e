"""The record filters at the extremes of the BAM fields, in all three header decoders, against the oracle.

plan_head's arithmetic is written to survive any field value (`s - 2u <= glen - 4u - L`, TLEN negated in 64 bits,
pss_len_never), and decode_hdr / decode_hdr_lds / decode_hdr_lds32 reach it through slightly different 32- and 64-bit
sums.  One small dataset of crafted records pins them to one answer: contigs of 1 to N + 5 bases, POS-1 from -1 to
2^31-1, CIGAR lengths up to 2^28-1, TLEN up to +-(2^31-1) and -2^31, MAPQ 254 / 255, SEQ *, -l / -L beyond 2^32.

Every crafted record is a TWIN with one field changed: the twin is a candidate in every respect, and the fixture
asserts on the CPU oracle that every twin is tallied.  The dataset goes through submit() under KERNEL_SIMPLE (decode_hdr),
KERNEL_TILED (decode_hdr_lds) and KERNEL_AUTO (-r 1 and -r 5: tally_compact, decode_hdr_lds32) with k-mers fused;
tables, k-mer tables and status counters must equal the oracle's on the SAM text of the same records.  The one record
with TLEN = -2^31 is kept out of the SAM (abs() of it is undefined in the reference and in the oracle); no contig holds
2^31 bases, so it is filtered, and the counters are expected accordingly.  There is no contig of length 0: on one the
reference's own end test (`aln_end + 2 > len - 1`, unsigned) passes every read and the oracle would read past the
buffer.  Bit-exact (integer work)."""
import os
import subprocess
from dataclasses import replace

import numpy as np
import pytest

import __graft_entry__ as ge
import pssbam_testlib as tl

pytestmark = pytest.mark.gpu

ROWS = (1, 5, 25)
KS = (1, 2, 5, 6)
BIG = 3000
L0 = 30                                   # the twins' length: a candidate at every -r of ROWS
SMALL = sorted({1, 3, 4, 5} | {n + d for n in ROWS for d in (3, 4, 5)})
I32_MAX, CIG_MAX = (1 << 31) - 1, (1 << 28) - 1
BEYOND_U32 = (1 << 32) + 5
PAIR1, PAIR2R = 0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80 | 0x10


def clean(rng, n: int) -> str:
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))


def build():
    """(contigs, refs, recs, twins, tlen_min): recs in SAM-able form, tlen_min the one record that is not"""
    rng = np.random.default_rng(9801)
    contigs = [("big", clean(rng, BIG))] + [(f"c{n}", clean(rng, n)) for n in SMALL]
    text = dict(contigs)
    refs = [(nm, len(s)) for nm, s in contigs]
    recs, twins = [], []
    count = [0]

    def read(rname, s, L, flag=0, tlen=0, mapq=40, seq=None):
        count[0] += 1
        ref = text[rname]
        if seq is None:
            seq = (ref[max(s, 0):max(s, 0) + L] if 0 <= s < len(ref) else "").ljust(L, "A")[:L]
        return tl.Rec(qname=f"x{count[0]:04d}" + "y" * (count[0] % 5), flag=flag, rname=rname, pos=s + 1, mapq=mapq, cigar=[(L, "M")],
                      tlen=tlen, seq=seq, qual="*" if seq == "*" else "I" * len(seq))

    def vary(twin, **change):
        """the twin with one field changed (a name of its own); SEQ follows POS only so that the SAM text stays sane"""
        count[0] += 1
        twins.append(twin)
        recs.append(replace(twin, qname=f"v{count[0]:04d}" + "z" * (count[0] % 7), **change))

    # the twins themselves: unpaired, first mate, second mate on the reverse strand
    U = read("big", 100, L0)
    P1 = read("big", 140, L0, PAIR1, L0)
    P2 = read("big", 180, L0, PAIR2R, -L0)
    for t in (U, P1, P2):
        vary(t)
    # 1. POS-1 on the big contig
    starts = [-1, 0, 1, 2, 3, *range(BIG - L0 - 3, BIG - L0 + 2), BIG - 1, BIG, BIG + 1, 1 << 28, I32_MAX - 1, I32_MAX]
    for t in (U, P1, P2):
        for s in starts:
            vary(t, pos=s + 1)
    # 2. small contigs: L in {1, N}; every start at which a clause of  s >= 2 && s + L + 2 <= glen  flips.  The twin is the
    #    same read at start 2 of a contig of L + 4 bases (c5 for L = 1, c{N+4} for L = N); its SEQ copies that contig.
    for L in sorted({1, *ROWS}):
        home = f"c{L + 4}"
        twin = read(home, 2, L)
        vary(twin)
        for glen in SMALL:
            for s in sorted({0, 1, 2, 3, *(x for x in range(glen - L - 3, glen - L + 2) if x >= 0)}):
                if (f"c{glen}", s) != (home, 2):
                    vary(twin, rname=f"c{glen}", pos=s + 1)
        ptwin = read(home, 2, L, PAIR1, -L)
        for glen in (L + 3, L + 4, L + 5):
            for s in (1, 2, 3):
                vary(ptwin, rname=f"c{glen}", pos=s + 1)
    # 3. CIGAR <c>M
    for t in (U, P1, P2):
        for c in (1, L0 - 1, L0, L0 + 1, CIG_MAX):
            vary(t, cigar=[(c, "M")])
    # 4. TLEN of a paired read, under the twin's own CIGAR and under <|TLEN|>M (SEQ keeps its 30 bases)
    tlens = [0, *(sg * v for v in sorted({1, *(n - 1 for n in ROWS if n > 1), *ROWS, L0, CIG_MAX, I32_MAX}) for sg in (1, -1))]
    for t in (P1, P2):
        for v in tlens:
            vary(t, tlen=v)
            if 1 <= abs(v) <= CIG_MAX:
                vary(t, tlen=v, cigar=[(abs(v), "M")])
        vary(t, tlen=I32_MAX, pos=1)                      # with every start that could let 2^31-1 bases "fit"
        vary(t, tlen=-I32_MAX, pos=3)
    tlen_min = replace(P1, qname="tlen_min", tlen=-(1 << 31), cigar=[(L0 + 1, "M")])      # (31M over 30 bases: fragkon filters it too)
    twins.append(P1)
    # 5. MAPQ
    for t in (U, P1):
        for q in (0, 36, 37, 254, 255):
            vary(t, mapq=q)
    # 6. SEQ *: strlen("*") is 1
    star = read("big", 300, 1)
    vary(star)
    vary(star, seq="*", qual="*")                         # a candidate at -r 1 whose only base is not A/C/G/T
    vary(P1, seq="*", qual="*")
    vary(P2, seq="*", qual="*")
    vary(U, seq="*", qual="*")                            # unpaired: L becomes 1, the CIGAR no longer matches
    # 7. fragkon's edges: starts k/2 - 1 and k/2, ends glen - k/2 - 1 .. glen - k/2 + 1 (pss filters most of them)
    for k in KS:
        for s in {k // 2 - 1, k // 2} | {BIG - L0 - k // 2 + d for d in (-1, 0, 1)}:
            if s >= 0:
                vary(U, pos=s + 1)
                vary(P1, pos=s + 1)
                vary(P2, pos=s + 1)
    return contigs, refs, recs, twins, tlen_min


@pytest.fixture(scope="module")
def pkg():
    p = ge.load_pkg()
    assert p.LIB_HIP.exists(), "libpssbam_hip.so missing: the HIP path must be built, there is no fallback"
    return p


@pytest.fixture(scope="module")
def data(oracle, tmp_path_factory):
    contigs, refs, recs, twins, tlen_min = build()
    tmp = tmp_path_factory.mktemp("extremes")
    loaded = tl.loaded_contigs(contigs)
    g = oracle.genome_from_arrays(loaded)
    tl.write_sam(tmp / "all.sam", refs, recs)
    # every twin is tallied: at -r 1 all of them, at the larger -r those that are long enough
    uniq = list({id(t): t for t in twins}.values())
    for n in ROWS:
        sel = [t for t in uniq if (abs(t.tlen) if t.flag & 1 else len(t.seq)) >= n]
        tl.write_sam(tmp / "twins.sam", refs, sel)
        st = oracle.pss(g, tmp / "twins.sam", tl.PssOpts(region_len=n))[2]
        assert len(sel) >= 4 and st[tl.ST_OK] == len(sel), (n, st)
    assert 300 < len(recs) < 1000 and len(uniq) >= 8
    everything = recs[:len(recs) // 2] + [tlen_min] + recs[len(recs) // 2:]
    d = dict(contigs=contigs, refs=refs, recs=recs, everything=everything, loaded=loaded, raw=tl.raw_records(refs, everything), g=g, tmp=tmp, memo={})
    yield d
    oracle.free_genome(g)


def expectation(oracle, d, po: tl.PssOpts, fo: tl.FkOpts):
    key = (repr(po), repr(fo))
    if key not in d["memo"]:
        wf, wr, st = oracle.pss(d["g"], d["tmp"] / "all.sam", po)
        k5, k3, kst = oracle.fragkon(d["g"], d["tmp"] / "all.sam", fo)
        assert st[tl.ST_PARSE_SKIP] == 0 and st[tl.ST_NO_CONTIG] == 0
        # + the TLEN = -2^31 record: filtered by both tallies
        stats = dict(records=len(d["recs"]) + 1, parse_skip=0, no_contig=0, pss_ok=int(st[tl.ST_OK]), pss_filtered=int(st[tl.ST_FILTERED]) + 1,
                     kmer_ok=int(kst[tl.ST_OK]), kmer_filtered=int(kst[tl.ST_FILTERED]) + 1, kmer_fail=int(kst[tl.ST_KMER_FAIL]))
        d["memo"][key] = (wf, wr, k5, k3, stats)
    return d["memo"][key]


def run(pkg, oracle, d, kernel: str, po: tl.PssOpts, fo: tl.FkOpts):
    wf, wr, k5, k3, stats = expectation(oracle, d, po, fo)
    eng = pkg.Engine(pss=dict(region_len=po.region_len, min_read_len=po.min_read_len, max_read_len=po.max_read_len, min_mq=po.min_mq),
                     kmer=dict(klen=fo.klen, min_read_len=fo.min_read_len, max_read_len=fo.max_read_len, min_mq=fo.min_mq),
                     kernel={"SIMPLE": pkg.KERNEL_SIMPLE, "TILED": pkg.KERNEL_TILED, "AUTO": pkg.KERNEL_AUTO}[kernel])
    try:
        eng.set_genome_arrays(d["loaded"])
        eng.set_references([nm for nm, _ in d["refs"]])
        eng.submit(d["raw"])
        tot = eng.finish()
    finally:
        eng.close()
    same = lambda a, b: np.array_equal(a, np.asarray(b).astype(np.uint64))     # noqa: E731
    assert same(tot.fwd, wf) and same(tot.rev, wr), "substitution tables differ"
    assert same(tot.k5, k5) and same(tot.k3, k3), "k-mer tables differ"
    assert {k: tot.stats[k] for k in stats} == stats
    return wf, wr, stats


@pytest.mark.parametrize("kernel", ["SIMPLE", "TILED", "AUTO"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", ROWS)
def test_three_decoders_one_answer(pkg, oracle, data, n, k, kernel):
    wf, wr, stats = run(pkg, oracle, data, kernel, tl.PssOpts(region_len=n), tl.FkOpts(klen=k))
    assert wf[2:].any() and wr[2:].any() and 10 < stats["pss_ok"] < stats["pss_filtered"] and 10 < stats["kmer_ok"]


LIMITS = {"q37": dict(min_mq=37), "l0_Lbeyond": dict(min_read_len=0, max_read_len=BEYOND_U32), "lbeyond": dict(min_read_len=BEYOND_U32),
          "l2_L250M": dict(min_read_len=2, max_read_len=250000000), "l30_L30": dict(min_read_len=L0, max_read_len=L0)}


@pytest.mark.parametrize("kernel", ["SIMPLE", "TILED", "AUTO"])
@pytest.mark.parametrize("limits", list(LIMITS))
def test_mapq_and_length_limits(pkg, oracle, data, limits, kernel):
    """-q 37 against MAPQ 0 / 36 / 37 / 254 / 255; -l and -L (and fragkon's) at 0, 2^32 + 5 and 250000000"""
    kw = LIMITS[limits]
    _, _, stats = run(pkg, oracle, data, kernel, tl.PssOpts(region_len=1, **kw), tl.FkOpts(klen=2, **kw))
    plain = expectation(oracle, data, tl.PssOpts(region_len=1), tl.FkOpts(klen=2))[4]
    if limits == "lbeyond":
        assert stats["pss_ok"] == 0 and stats["kmer_ok"] == 0
    elif limits == "l0_Lbeyond":
        assert stats == plain
    else:
        assert 0 < stats["pss_ok"] < plain["pss_ok"] and 0 < stats["kmer_ok"] < plain["kmer_ok"]


def test_command_line_routes(pkg, oracle, data, tmp_path):
    """bin/pss-bam on the BAM of the same records (the TLEN = -2^31 one included): the counts file of the default feed and
    of the host reader are identical and hold the oracle's tables"""
    fa, aln = tmp_path / "g.fa", tmp_path / "in.bam"
    tl.write_fasta(fa, data["contigs"])
    tl.write_bam(aln, data["refs"], data["everything"])
    exe = pkg.PKG_DIR / "bin" / "pss-bam"
    outs = []
    for env in ({}, {"PSSBAM_DEVICE_INFLATE": "0"}):
        pr = subprocess.run([str(exe), "-F", str(fa), "-B", str(aln), "-o", str(tmp_path / "out"), "-r", "5"], capture_output=True, text=True,
                            env={**os.environ, **env}, timeout=300)
        assert pr.returncode == 0, pr.stderr
        outs.append((tmp_path / "out.pss.counts.txt").read_text())
    assert outs[0] == outs[1]
    wf, wr, _ = oracle.pss(data["g"], data["tmp"] / "all.sam", tl.PssOpts(region_len=5))
    gf, gr = tl.parse_counts_text(outs[0])
    assert np.array_equal(gf, wf) and np.array_equal(gr, wr) and wf[2:].any()

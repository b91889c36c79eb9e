"""Crafted BAM streams and BGZF block layouts for the device record index (the bgzf_chain_* kernels of
csrc/inflate_kernels.h and the host side of the feed in csrc/bgzf_api.h).  No GPU in here.

The reference for every test is walk(): the serial block_size walk of the inflated stream.  Everything else helps to PLACE
bytes so that a named branch of the kernels is reached -- plausible() is the SAM-spec layout arithmetic the kernels judge a
candidate by, spec() restates the first pass (every block's own guess) and broken_links() the link check behind it,
super_batches() restates how the Python wrapper and the engine cut a stream into submits, super-batches and tally
sub-batches.  test_feed_chain_host.py asserts with them that each construction is what it claims to be; none of them is an
expected value of a GPU test.

Every record of these streams is one the engine keeps and tallies (unpaired, mapped, <L>M, inside its contig, MAPQ 40, an
upper-case ACGT reference), so the record sink must deliver the whole record stream.  Records that host a trap carry a B:C
aux array of 0xFF bytes -- a byte value at which nothing is plausible -- into which fake records are planted."""
from __future__ import annotations

import struct
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import pssbam_testlib as tl

MAX_RECORD = 1 << 24          # CHAIN_MAX_RECORD: block_size above it raises PSSBAM_FEED_RAGGED
NEAR_END = 36 + 256           # the kernels judge a record by its length alone this close to the end of a super-batch's data
TRIES = 4                     # candidates bgzf_chain_spec tries per block
SUPER_DEFAULT = 4400 << 20    # FEED_OUT_TARGET
SUB_DEFAULT = 3584 << 20      # FEED_SUB_MAX
CONTIG = "chr1"
IDX = {CONTIG: 0}
N_REF = 1
TRAILER = b"XZZbehind the array\0"
MARGIN = 64                   # no read within so many bases of a contig end (a read without a flanking reference base is not tallied)


def u32(buf, o: int) -> int:
    return struct.unpack_from("<I", buf, o)[0]


# ----------------------------------------------------------------------------------------------------------------------
# records and streams
# ----------------------------------------------------------------------------------------------------------------------
def genome(seed: int, length: int = 30000):
    rng = np.random.default_rng(seed)
    text = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, length))
    return [(CONTIG, text)], [(CONTIG, length)]


def reads(seed: int, contigs, n: int, lo: int = 30, hi: int = 90, tag: str = "r", span: int | None = None) -> list[tl.Rec]:
    """n records the engine keeps: unpaired, mapped, <L>M inside the contig, MAPQ 40, a few substitutions.
    span: starts are drawn from the first `span` positions only (duplicates of position, length and strand then occur)."""
    rng = np.random.default_rng(seed)
    text = contigs[0][1]
    out = []
    for i in range(n):
        L = int(rng.integers(lo, hi + 1))
        s = MARGIN + int(rng.integers(0, min(span or len(text), len(text) - L + 1 - 2 * MARGIN)))
        seq = list(text[s:s + L])
        for j in np.flatnonzero(rng.random(L) < 0.03):
            seq[int(j)] = "ACGT"[int(rng.integers(0, 4))]
        qual = "".join(chr(33 + int(q)) for q in rng.integers(2, 42, size=L))
        out.append(tl.Rec(qname=f"{tag}{i:06d}", flag=0x10 if rng.random() < 0.5 else 0, rname=CONTIG, pos=s + 1, mapq=40,
                          cigar=[(L, "M")], seq="".join(seq), qual=qual))
    return out


def array_record(rec: tl.Rec, n: int | None = None, block_size: int | None = None, trailer: bool = False) -> tuple[bytes, int]:
    """tl.bam_record(rec) with a B:C aux array of n 0xFF bytes behind it (or as many as make its block_size `block_size`),
    and with `trailer` a Z tag behind the array.  Returns the record and the array's offset in it."""
    base = tl.bam_record(rec, IDX)
    tail = TRAILER if trailer else b""
    if n is None:
        n = block_size - (len(base) - 4) - 8 - len(tail)
    assert n >= 0
    body = base[4:] + b"XBBC" + struct.pack("<I", n) + b"\xff" * n + tail
    return struct.pack("<I", len(body)) + body, len(base) + 8


def stream(refs, recs) -> tuple[bytes, list[bytes], list[int]]:
    """recs: tl.Rec or ready record bytes.  Returns the header bytes, the records' bytes and their start offsets in
    header + records (one more than records: the last is the stream's length)."""
    head = tl.bam_bytes(refs, [])
    bodies = [r if isinstance(r, (bytes, bytearray)) else tl.bam_record(r, IDX) for r in recs]
    starts = [len(head)]
    for b in bodies:
        starts.append(starts[-1] + len(b))
    return head, bodies, starts


def layout(raw: bytes, cuts, level: int = 1, eof_at=()) -> tuple[bytes, list[int]]:
    """BGZF bytes with a block boundary at every offset in `cuts` (a repeated offset, 0 or len(raw) gives an empty block; an
    empty block at an offset in eof_at is the EOF marker itself), closed by the EOF block.  Also returns the blocks' bounds in
    `raw`, the closing EOF block included."""
    pts = [0] + sorted(int(c) for c in cuts) + [len(raw)]
    assert pts[1] >= 0 and pts[-2] <= len(raw)
    out = []
    for a, b in zip(pts[:-1], pts[1:]):
        assert b - a <= 0xFF00, (a, b)
        out.append(tl.BGZF_EOF if a == b and a in eof_at else tl.bgzf_block(bytes(raw[a:b]), level))
    return b"".join(out) + tl.BGZF_EOF, pts + [len(raw)]


def grid(n: int, step: int, holes=(), extra=()) -> list[int]:
    """cuts every `step` bytes of an n-byte stream, none inside the half-open ranges `holes`, plus `extra`"""
    cuts = {c for c in range(step, n, step) if not any(a <= c < b for a, b in holes)}
    return sorted(cuts | {int(x) for x in extra})


def walk(raw, at: int) -> tuple[list[tuple[int, int]], int]:
    """the serial block_size walk: (start, end) of every whole record from `at`, and where it stopped (the stream's length,
    or the start of a record the stream ends inside)"""
    out, o = [], at
    while o + 4 <= len(raw):
        bs = u32(raw, o)
        assert bs >= 32, (o, bs)
        if o + 4 + bs > len(raw):
            break
        out.append((o, o + 4 + bs))
        o += 4 + bs
    return out, o


def plausible(buf, off: int, n_ref: int = N_REF, end: int | None = None) -> bool:
    """SAM spec 4.2 layout arithmetic and value ranges of a record that would start at `off`, judged with the bytes below
    `end` (what plausible_record of csrc/inflate_kernels.h sees)"""
    end = len(buf) if end is None else end
    avail = end - off
    if avail < 36:
        return False
    bs, ref_id, pos, w3, w4, l_seq, next_ref, next_pos = struct.unpack_from("<IiiIIIii", buf, off)
    l_name, n_cig = w3 & 0xFF, w4 & 0xFFFF
    if bs < 32 or bs > MAX_RECORD or l_name == 0:
        return False
    if ref_id < -1 or ref_id >= n_ref or next_ref < -1 or next_ref >= n_ref or pos < -1 or next_pos < -1:
        return False
    if l_seq > bs or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return False
    if 36 + l_name <= avail and buf[off + 36 + l_name - 1] != 0:
        return False
    return True


def plausible_offsets(buf, lo: int, hi: int, end: int | None = None) -> list[int]:
    return [c for c in range(lo, hi) if buf[c + 3] <= 1 and plausible(buf, c, N_REF, end)]


def chain(buf, off: int, end: int | None = None) -> tuple[int, int]:
    """how many plausible records follow one another from `off`, and where that chain stops"""
    end = len(buf) if end is None else end
    k = 0
    while off < end and plausible(buf, off, N_REF, end):
        off += 4 + u32(buf, off)
        k += 1
    return k, off


def spec(raw, bounds, first_start: int, end: int | None = None):
    """The first pass over one super-batch whose data is raw[:end] (bgzf_chain_spec): per block (a, n, e) -- the first record
    start the block guesses on its own (None: none), the records it claims, where the last of them ends."""
    end = len(raw) if end is None else end
    out = []
    for b, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        if b == 0:
            o, n = first_start, 0
            while o < hi and o + 4 <= end:
                o += 4 + u32(raw, o)
                n += 1
            out.append((first_start if n else None, n, o))
            continue
        got, c, tries = (None, 0, 0), lo, 0
        while tries < TRIES:
            while c < hi and not (c + 3 < end and raw[c + 3] <= 1 and plausible(raw, c, N_REF, end)):
                c += 1
            if c >= hi:
                break
            tries += 1
            o, k, extra, good, end_in = c, 0, 0, True, c
            while o + 4 <= end:
                bs = u32(raw, o)
                if not (plausible(raw, o, N_REF, end) or (end - o < NEAR_END and 32 <= bs <= MAX_RECORD)):
                    good = False
                    break
                if o < hi:
                    k, end_in = k + 1, o + 4 + bs
                else:
                    extra += 1
                    if extra >= 2:
                        break
                o += 4 + bs
                if o >= end:
                    break
            if good and k:
                got = (c, k, end_in)
                break
            c += 1
        out.append(got)
    return out


def broken_links(raw, guesses, end: int | None = None) -> list[int]:
    """the blocks whose chain does not end where the next claimed record starts (the first bgzf_chain_verify pass)"""
    end = len(raw) if end is None else end
    nexta, run = [None] * (len(guesses) + 1), None
    for b in range(len(guesses) - 1, -1, -1):
        if guesses[b][0] is not None:
            run = guesses[b][0]
        nexta[b] = run
    out = []
    for b, (_, n, e) in enumerate(guesses):
        if not n:
            continue
        if nexta[b + 1] is not None:
            if e != nexta[b + 1]:
                out.append(b)
        elif e < end and end - e >= 4:
            bs = u32(raw, e)
            if not (32 <= bs <= MAX_RECORD and e + 4 + bs > end):
                out.append(b)
    return out


def super_batches(bounds, head_len: int, max_batch: int = 1 << 30, super_bytes: int | None = None,
                  sub_bytes: int | None = None) -> list[list[tuple[int, int]]]:
    """How Engine.submit_bgzf and the engine cut the blocks: per super-batch the (start, end) stream offsets of its tally
    sub-batches.  Blocks that are all header are skipped; a submit takes blocks while they inflate to at most max_batch; a
    super-batch is flushed behind the submit that fills it (a third of the target for the stream's first one); a new
    sub-batch begins where the record bytes would pass sub_bytes.  Holds for submits below 64 MiB and super-batches of fewer
    than 8192 blocks, which is every stream of this module."""
    target = max(1 << 20, super_bytes) if super_bytes else SUPER_DEFAULT
    sub_max = min(SUB_DEFAULT, max(65536, sub_bytes)) if sub_bytes else SUB_DEFAULT
    n = len(bounds) - 1
    i, skip = 0, head_len
    while i < n and skip >= bounds[i + 1] - bounds[i] and (skip > 0 or bounds[i + 1] == bounds[i]):
        skip -= bounds[i + 1] - bounds[i]
        i += 1
    out, first = [], i
    while i < n:
        j = i
        while j < n and bounds[j + 1] - bounds[i] <= max_batch:
            j += 1
        j = max(j, i + 1)
        if bounds[j] - bounds[first] >= (target // 3 if not out else target) or j == n:
            subs, s0, used = [], first, 0
            for b in range(first, j):
                if used + bounds[b + 1] - bounds[b] > sub_max:
                    subs.append((bounds[s0], bounds[b]))
                    s0, used = b, 0
                used += bounds[b + 1] - bounds[b]
            subs.append((bounds[s0], bounds[j]))
            out.append(subs)
            first = j
        i = j
    return out


def super_ends(*a, **kw) -> list[int]:
    return [sb[-1][1] for sb in super_batches(*a, **kw)]


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Fake:
    at: int            # where the planted chain begins
    n: int             # plausible fake records it chains for
    on_boundary: bool  # whether it stops on a real record boundary


@dataclass
class Case:
    name: str
    contigs: list
    refs: list
    raw: bytes                 # header + records: the inflated stream
    head_len: int
    cuts: list
    n_records: int             # the whole records the stream was built from
    eof_at: tuple = ()
    level: int = 1
    flags: int = 0
    env: dict = field(default_factory=dict)      # PSSBAM_FEED_SUPER_BYTES / _SUB_BYTES of the run
    max_batch: int = 1 << 30
    fakes: list = field(default_factory=list)
    repair: bool = False       # PSSBAM_FEED_REPAIR=0 must raise PSSBAM_FEED_RAGGED on this input
    note: dict = field(default_factory=dict)     # offsets the host test asserts on

    def bgzf(self):
        """(BGZF bytes, block bounds) of the stream under the case's cuts"""
        if "_bgzf" not in self.__dict__:
            self.__dict__["_bgzf"] = layout(self.raw, self.cuts, self.level, self.eof_at)
        return self.__dict__["_bgzf"]

    def supers(self):
        """the super-batches (and their sub-batches) the case's run is cut into"""
        e = {k: int(v) for k, v in self.env.items()}
        return super_batches(self.bgzf()[1], self.head_len, self.max_batch, e.get("PSSBAM_FEED_SUPER_BYTES"),
                             e.get("PSSBAM_FEED_SUB_BYTES"))


class Build:
    """a stream under construction: records (some hosting an 0xFF array) and what is planted into the arrays"""

    def __init__(self, seed: int, n: int, hosts: dict | None = None, lo: int = 30, hi: int = 90, span: int | None = None):
        self.seed = seed
        self.contigs, self.refs = genome(seed)
        recs = reads(seed + 1, self.contigs, n, lo, hi, span=span)
        bodies, self.arrays = [], {}
        for i, r in enumerate(recs):
            if hosts and i in hosts:
                b, at = array_record(r, **hosts[i])
                self.arrays[i] = at
                bodies.append(b)
            else:
                bodies.append(tl.bam_record(r, IDX))
        head, bodies, self.starts = stream(self.refs, bodies)
        self.head_len = len(head)
        self.raw = bytearray(head + b"".join(bodies))
        self.arrays = {i: (self.starts[i] + at, u32(self.raw, self.starts[i] + at - 4)) for i, at in self.arrays.items()}
        self.n_fake = 0

    def array(self, i: int) -> tuple[int, int]:
        """(first byte, one past the last byte) of host i's array"""
        return self.arrays[i][0], self.arrays[i][0] + self.arrays[i][1]

    def fake_chain(self, k: int, lo: int = 30, hi: int = 90) -> bytes:
        """k fresh records (of no stream) back to back"""
        self.n_fake += 1
        return b"".join(tl.bam_record(r, IDX) for r in reads(self.seed + 100 + self.n_fake, self.contigs, k, lo, hi, tag="f"))

    def plant(self, at: int, payload: bytes):
        assert self.raw[at:at + len(payload)] == b"\xff" * len(payload), "fake records go into an array's filler"
        self.raw[at:at + len(payload)] = payload

    def case(self, name: str, cuts, **kw) -> Case:
        whole = sum(1 for e in self.starts[1:] if e <= len(self.raw))
        return Case(name, self.contigs, self.refs, bytes(self.raw), self.head_len, list(cuts), whole, **kw)


SUPER_1M = {"PSSBAM_FEED_SUPER_BYTES": "1048576"}


@lru_cache(maxsize=None)
def tiny_blocks() -> Case:
    """case 1: blocks of 1, 3, 4, 35, 36 and 37 bytes; empty blocks mid-stream, an EOF block mid-stream, an empty last block"""
    b = Build(101, 60)
    cuts, o, k = [], 0, 0
    sizes = (1, 3, 4, 35, 36, 37, 4, 1, 37, 3, 36, 35)
    while o + sizes[k % len(sizes)] < len(b.raw):
        o += sizes[k % len(sizes)]
        cuts.append(o)
        k += 1
    mid, eof = cuts[len(cuts) // 3], cuts[2 * len(cuts) // 3]
    for i in (10, 30, 50):                   # a length word over four blocks
        cuts = sorted(set(cuts) | {b.starts[i] + 1, b.starts[i] + 2, b.starts[i] + 3})
    cuts += [mid, mid, eof, len(b.raw)]
    return b.case("tiny_blocks", cuts, eof_at=(eof,), note=dict(empty=mid, eof=eof))


@lru_cache(maxsize=None)
def false_start_inside() -> Case:
    """case 2: a fake chain that begins 40 bytes into a block, the true record start later in the same block"""
    b = Build(102, 400, {200: dict(n=600)})
    a0, a1 = b.array(200)
    fake = b.fake_chain(3)
    at = a1 - len(fake)                      # the chain ends with the host record: it runs on into the true records
    b.plant(at, fake)
    blk = at - 40
    assert blk >= a0
    cuts = grid(len(b.raw), 700, holes=[(blk, b.starts[201] + 300)], extra=[blk])
    return b.case("false_start_inside", cuts, fakes=[Fake(at, 3, True)], repair=True,
                  note=dict(block=blk, true_start=b.starts[201], host=200))


@lru_cache(maxsize=None)
def four_decoys() -> Case:
    """case 3: four plausible headers whose chains fail, in front of the true start in one block"""
    b = Build(103, 400, {200: dict(n=900)})
    a0, _ = b.array(200)
    fakes = []
    for k in range(4):
        at = a0 + 100 + 200 * k
        b.plant(at, b.fake_chain(1))         # one record, 0xFF behind it
        fakes.append(Fake(at, 1, False))
    blk = a0 + 50
    cuts = grid(len(b.raw), 700, holes=[(blk, b.starts[201] + 300)], extra=[blk])
    return b.case("four_decoys", cuts, fakes=fakes, repair=True, note=dict(block=blk, true_start=b.starts[201], host=200))


def _block_at_fake(b: Build, host: int, k: int = 8, into: int = 50) -> Fake:
    """plants k fake records `into` bytes into host's array; the caller cuts a block there"""
    a0, a1 = b.array(host)
    fake = b.fake_chain(k)
    assert a0 + into + len(fake) + 8 <= a1
    b.plant(a0 + into, fake)
    return Fake(a0 + into, k, False)


@lru_cache(maxsize=None)
def broken_behind_anchor() -> Case:
    """case 4a: the fake chain is block 1, the host record the first of the stream"""
    b = Build(104, 300, {0: dict(n=1500)})
    f = _block_at_fake(b, 0)
    cuts = grid(len(b.raw), 700, holes=[(0, f.at + 300)], extra=[f.at, f.at + 300])
    return b.case("broken_behind_anchor", cuts, fakes=[f], repair=True, note=dict(host=0))


@lru_cache(maxsize=None)
def broken_far_apart() -> Case:
    """case 4b: broken links at a block index >= 64 and again more than 64 blocks later"""
    b = Build(105, 1400, {700: dict(n=1500), 1300: dict(n=1500)})
    fs = [_block_at_fake(b, 700), _block_at_fake(b, 1300)]
    cuts = grid(len(b.raw), 700, extra=[f.at for f in fs])
    return b.case("broken_far_apart", cuts, fakes=fs, repair=True, note=dict(hosts=(700, 1300)))


@lru_cache(maxsize=None)
def broken_twice_in_a_row() -> Case:
    """case 4c: two neighbouring host records, a block at each one's fake chain: two consecutive links are broken"""
    b = Build(106, 400, {200: dict(n=800), 201: dict(n=800)})
    fs = []
    for h in (200, 201):
        _, a1 = b.array(h)
        fake = b.fake_chain(3)
        b.plant(a1 - len(fake), fake)        # ends with the host: block b+1 goes on to claim the TRUE record 201
        fs.append(Fake(a1 - len(fake), 3, True))
    cuts = grid(len(b.raw), 700, holes=[(b.starts[200], b.starts[202] + 100)], extra=[f.at for f in fs])
    return b.case("broken_twice_in_a_row", cuts, fakes=fs, repair=True, note=dict(hosts=(200, 201)))


@lru_cache(maxsize=None)
def broken_at_super_end() -> Case:
    """case 4d: the fake chain is the last block of the first super-batch and its first record runs past that super-batch's
    data: the first verify pass takes the fake record for the tail"""
    env, max_batch, n = dict(SUPER_1M), 7000, 4000
    plain = Build(107, n)
    end0 = super_ends(layout(plain.raw, grid(len(plain.raw), 700))[1], plain.head_len, max_batch, 1 << 20)[0]
    host = max(i for i in range(n) if plain.starts[i] <= end0 - 1000)
    b = Build(107, n, {host: dict(n=4000)})
    at = end0 - 350
    fake = b.fake_chain(4, 300, 400)         # long records: the first starts more than NEAR_END bytes before the end
    b.plant(at, fake)
    cuts = grid(len(b.raw), 700, extra=[at])
    return b.case("broken_at_super_end", cuts, env=env, max_batch=max_batch, fakes=[Fake(at, 4, False)], repair=True,
                  note=dict(host=host, end0=end0, first_len=4 + u32(fake, 0)))


@lru_cache(maxsize=None)
def inside_long_record(trailer: bool) -> Case:
    """case 5: a record over six blocks, a fake chain in a block that lies entirely inside it; the chain ends with the
    array, which is the host record's end or -- trailer -- a Z tag short of it"""
    b = Build(108, 400, {200: dict(n=3500, trailer=trailer)})
    _, a1 = b.array(200)
    fake = b.fake_chain(10)
    at = a1 - len(fake)
    b.plant(at, fake)
    cuts = grid(len(b.raw), 700, extra=[at])
    return b.case(f"inside_long_record_{'z' if trailer else 'end'}", cuts, fakes=[Fake(at, 10, not trailer)], repair=True,
                  note=dict(host=200))


def _with_long(seed: int, before: int, after: int, block_size: int):
    contigs, refs = genome(seed)
    recs = reads(seed + 1, contigs, before + 1 + after)
    bodies = [tl.bam_record(r, IDX) for r in recs]
    bodies[before], at = array_record(recs[before], block_size=block_size)
    head, bodies, starts = stream(refs, bodies)
    return contigs, refs, head, bodies, starts, starts[before] + at


@lru_cache(maxsize=None)
def record_2_5_mib(with_fakes: bool) -> Case:
    """case 6: a 2.5 MiB record under 1 MiB super-batches: super-batches in which no record starts, a carry that grows; with
    fake chains at three block starts of the middle super-batch (blocks of 300 bytes, which the chains outrun)"""
    contigs, refs, head, bodies, starts, a0 = _with_long(109, 150, 150, 2621440)
    raw = bytearray(head + b"".join(bodies))
    fakes = []
    if with_fakes:
        for k, at in enumerate((800000, 850000, 900000)):
            fake = b"".join(tl.bam_record(r, IDX) for r in reads(900 + k, contigs, 5, tag="f"))
            assert raw[at:at + len(fake)] == b"\xff" * len(fake)
            raw[at:at + len(fake)] = fake
            fakes.append(Fake(at, 5, False))
    return Case(f"record_2_5_mib_{'fakes' if with_fakes else 'plain'}", contigs, refs, bytes(raw), len(head),
                grid(len(raw), 5000, extra=[f.at + 300 for f in fakes]), 301, env=dict(SUPER_1M), max_batch=65536, fakes=fakes, repair=with_fakes, note=dict(long=150))


@lru_cache(maxsize=2)
def record_16_mib(over: int) -> Case:
    """case 7: block_size == (1 << 24) + over between short records, one super-batch"""
    contigs, refs, head, bodies, _, _ = _with_long(110, 50, 50, (1 << 24) + over)
    raw = head + b"".join(bodies)
    return Case(f"record_16_mib_plus_{over}", contigs, refs, raw, len(head), grid(len(raw), 0xFF00), 101, flags=2 if over else 0,
                note=dict(long=50))


@lru_cache(maxsize=None)
def break_streams(cut_inside: bool):
    """case 8: stream X (cut inside its last record, or whole), stream Y with a header of its own, and Y's records alone in
    blocks of their own (no header: the bytes X's cut record still wants would be Y's first)"""
    x = Build(111, 300)
    end = x.starts[300] - 37 if cut_inside else x.starts[300]
    x.raw = x.raw[:end]
    cx = x.case(f"break_x_{'cut' if cut_inside else 'whole'}", grid(end, 700), flags=8 if cut_inside else 0)
    recs = reads(113, x.contigs, 200, tag="y")     # (one genome for both)
    head, bodies, _ = stream(x.refs, recs)
    raw = head + b"".join(bodies)
    cy = Case("break_y", x.contigs, x.refs, raw, len(head), grid(len(raw), 700), 200)
    body = b"".join(bodies)
    cy0 = Case("break_y_headerless", x.contigs, x.refs, body, 0, grid(len(body), 700), 200)
    return cx, cy, cy0


SUBS = {"PSSBAM_FEED_SUPER_BYTES": "1048576", "PSSBAM_FEED_SUB_BYTES": "131072"}


@lru_cache(maxsize=None)
def sub_ragged() -> Case:
    """case 9a: 2500 short reads in blocks of 5000 bytes, tally sub-batches of 128 KiB: records cross sub-batch bounds"""
    b = Build(114, 2500, span=1500)
    return b.case("sub_ragged", grid(len(b.raw), 5000), env=dict(SUBS), max_batch=40000)


@lru_cache(maxsize=None)
def sub_long() -> Case:
    """case 9b: the 2.5 MiB record of case 6 under 128 KiB sub-batches: sub-batches in which no record starts"""
    c = record_2_5_mib(False)
    return Case("sub_long", c.contigs, c.refs, c.raw, c.head_len, c.cuts, c.n_records, env=dict(SUBS), max_batch=65536, note=dict(c.note))


def records_of(case: Case) -> tuple[list[bytes], int]:
    """the whole records of the case's stream by the serial walk, and where the walk stopped"""
    spans, stop = walk(case.raw, case.head_len)
    return [case.raw[a:b] for a, b in spans], stop

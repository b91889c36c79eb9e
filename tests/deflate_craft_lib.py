"""A deflate WRITER for tests (RFC 1951), pure Python: it searches for nothing -- it is told the token list and the code
lengths, and writes exactly that.  With it the inflate paths (host/inflate_fast.c, csrc/inflate_kernels.h,
csrc/inflate_wave.h) are driven through the legal streams zlib's compressor never produces (what libdeflate, zlib-ng,
igzip and htsjdk's deflaters may write into a BAM) and through malformed ones, one defect at a time.

Tokens:  int 0..255        a literal
         (length, dist)    a match; (258, dist, True) codes length 258 as symbol 284 + extra bits 31
         ("sym", s)        the bare literal/length symbol s (malformed streams: 286, 287)
         ("dsym", length, s)   a length followed by the bare distance symbol s (30, 31)
         ("bits", v, n)    n raw bits (a bit pattern that is no code of an incomplete set)
Code lengths are lists indexed by symbol; a dynamic block's HLIT / HDIST are the lengths of the lists.
Header items (dynamic(..., header=[...])): an int is a code length written plainly, (16, n) / (17, n) / (18, n) a repeat
code with count n.

valid_cases() / invalid_cases() are the two corpora; tests/test_deflate_craft_host.py holds them to zlib and asserts
what each case claims to contain, so that an edit cannot hollow them out."""
import struct
import zlib
from pathlib import Path

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
BGZF_HEAD = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"


class BitWriter:
    """deflate's bit order: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):
        v, n = c
        r = 0
        for _ in range(n):
            r = (r << 1) | (v & 1)
            v >>= 1
        self.bits(r, n)

    @property
    def bitpos(self):
        return len(self.buf) * 8 + self.n

    def align(self, fill=0):
        if self.n:
            self.bits(0xFF if fill else 0, 8 - self.n)

    def getvalue(self, pad=0):
        out = bytearray(self.buf)
        if self.n:
            out.append((self.acc | ((0xFF << self.n) if pad else 0)) & 255)
        return bytes(out)


def canonical_codes(lens):
    """symbol -> (code, bits) for the nonzero lengths (RFC 1951 3.2.2)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for b in range(1, 17):
        c = (c + count[b - 1]) << 1
        nxt[b] = c
    codes = {}
    for s, l in enumerate(lens):
        if l:
            codes[s] = (nxt[l], l)
            nxt[l] += 1
    return codes


def kraft(lens, maxbits=15):
    """sum of 2^-l in units of 2^-maxbits: == 1 << maxbits for a complete code"""
    return sum(1 << (maxbits - l) for l in lens if l)


def complete_lens(n):
    """n >= 2 lengths of a complete code, as balanced as can be (ascending)"""
    assert n >= 2
    k = n.bit_length() - 1
    prof = [k] * (2 * (1 << k) - n) + [k + 1] * (2 * (n - (1 << k)))
    assert len(prof) == n and kraft(prof) == 1 << 15
    return prof


def comb_lens(n, k):
    """a complete code of n symbols: a comb 1, 2, ..., k and a balanced tail below it (ascending)"""
    assert 0 <= k <= n - 2
    prof = list(range(1, k + 1)) + [k + l for l in complete_lens(n - k)]
    assert len(prof) == n and max(prof) <= 15 and kraft(prof) == 1 << 15, (n, k)
    return prof


def deepest_comb(n, maxbits=15):
    """the comb with the longest teeth that n symbols allow within maxbits"""
    for k in range(min(n - 2, maxbits - 1), -1, -1):
        if k + (n - k - 1).bit_length() <= maxbits:
            return comb_lens(n, k)
    raise AssertionError(n)


def assign(order, profile, size):
    """code lengths by symbol: order[i] gets profile[i]"""
    assert len(order) == len(profile) and len(set(order)) == len(order)
    lens = [0] * size
    for s, l in zip(order, profile):
        lens[s] = l
    return lens


def len_symbol(length, alt258=False):
    if length == 258:
        return (284, 5, 31) if alt258 else (285, 0, 0)
    i = max(j for j in range(28) if LEN_BASE[j] <= length)
    assert length - LEN_BASE[i] < (1 << LEN_EXTRA[i])
    return 257 + i, LEN_EXTRA[i], length - LEN_BASE[i]


def dist_symbol(dist):
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    assert dist - DIST_BASE[i] < (1 << DIST_EXTRA[i])
    return i, DIST_EXTRA[i], dist - DIST_BASE[i]


def expand_header(items):
    out = []
    for it in items:
        if isinstance(it, int):
            out.append(it)
        elif it[0] == 16:
            out += [out[-1]] * it[1]
        else:
            out += [0] * it[1]
    return out


class Deflate:
    """one raw deflate stream, block by block; .blocks remembers what was asked for"""

    def __init__(self):
        self.w, self.blocks = BitWriter(), []

    def stored(self, data=b"", final=False, length=None, nlen=None):
        self.blocks.append(dict(kind="stored", data=bytes(data), bit_start=self.w.bitpos))
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        n = len(data) if length is None else length
        self.w.bits(n, 16)
        self.w.bits(n ^ 0xFFFF if nlen is None else nlen, 16)
        for b in data:
            self.w.bits(b, 8)
        return self

    def _emit(self, tokens, llc, dc):
        w = self.w
        for t in tokens:
            if isinstance(t, (int, np.integer)):
                w.code(llc[int(t)])
            elif t[0] == "sym":
                w.code(llc[t[1]])
            elif t[0] == "bits":
                w.bits(t[1], t[2])
            else:
                raw = t[0] == "dsym"
                length = t[1] if raw else t[0]
                s, e, x = len_symbol(length, (not raw) and len(t) > 2 and t[2])
                w.code(llc[s])
                w.bits(x, e)
                if raw:
                    w.code(dc[t[2]])
                else:
                    s, e, x = dist_symbol(t[1])
                    w.code(dc[s])
                    w.bits(x, e)

    def fixed(self, tokens, final=False, eob=True):
        self.blocks.append(dict(kind="fixed", tokens=list(tokens), ll_lens=FIXED_LL, d_lens=FIXED_D, bit_start=self.w.bitpos))
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        llc = canonical_codes(FIXED_LL)
        self._emit(tokens, llc, canonical_codes(FIXED_D))
        if eob:
            self.w.code(llc[256])
        return self

    def dynamic(self, tokens, ll_lens, d_lens, final=False, header=None, cl_lens=None, hclen=None, eob=True, strict=True):
        """strict=False: the header is written as given even if it is no legal description of the two codes"""
        hlit, hdist = len(ll_lens), len(d_lens)
        assert 257 <= hlit <= 288 and 1 <= hdist <= 32
        items = list(ll_lens) + list(d_lens) if header is None else list(header)
        if strict:
            assert expand_header(items) == list(ll_lens) + list(d_lens), "header does not describe the code lengths"
            assert hlit <= 286 and hdist <= 30
        used = [it if isinstance(it, int) else it[0] for it in items]
        if cl_lens is None:
            syms = sorted(set(used), key=lambda s: (-used.count(s), s))
            if len(syms) < 2:   # a one-symbol code-length code would be incomplete: give it a partner it never uses
                syms.append(next(s for s in (0, 18, 17, 16) if s not in syms))
            cl_lens = assign(syms, complete_lens(len(syms)), 19)
        need = max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1
        hclen = max(4, need) if hclen is None else hclen
        assert 4 <= hclen <= 19 and (hclen >= need or not strict)
        self.blocks.append(dict(kind="dynamic", tokens=list(tokens), ll_lens=list(ll_lens), d_lens=list(d_lens), header=items,
                                cl_lens=list(cl_lens), hclen=hclen, bit_start=self.w.bitpos))
        w = self.w
        w.bits(int(final), 1)
        w.bits(2, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        clc = canonical_codes(cl_lens)
        for it in items:
            if isinstance(it, int):
                w.code(clc[it])
            else:
                w.code(clc[it[0]])
                if it[0] == 16:
                    assert 3 <= it[1] <= 6
                    w.bits(it[1] - 3, 2)
                elif it[0] == 17:
                    assert 3 <= it[1] <= 10
                    w.bits(it[1] - 3, 3)
                else:
                    assert 11 <= it[1] <= 138
                    w.bits(it[1] - 11, 7)
        llc, dc = canonical_codes(ll_lens), canonical_codes(d_lens)
        self._emit(tokens, llc, dc)
        if eob:
            w.code(llc[256])
        return self

    def payload(self, pad=0):
        return self.w.getvalue(pad)

    def expected(self):
        out = bytearray()
        for b in self.blocks:
            if b["kind"] == "stored":
                out += b["data"]
            else:
                replay(b["tokens"], out)
        return bytes(out)


def replay(tokens, out=None):
    """LZ77 replay of a token list onto out (a bytearray): what any inflater must produce"""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            out.append(int(t))
        else:
            length, dist = t[0], t[1]
            assert 3 <= length <= 258 and 1 <= dist <= min(32768, len(out)), (length, dist, len(out))
            for _ in range(length):
                out.append(out[-dist])
    return out


def bgzf_frame(payload, data=None, isize=None, crc=None):
    """one BGZF block around a raw deflate payload; CRC and ISIZE are those of `data` unless given"""
    bsize = len(payload) + 25
    assert bsize <= 65535, "payload does not fit a BGZF block"
    if crc is None:
        crc = zlib.crc32(data) & 0xFFFFFFFF
    if isize is None:
        isize = len(data)
    return BGZF_HEAD + struct.pack("<H", bsize) + payload + struct.pack("<II", crc, isize)


def greedy_tokens(data):
    """a trivial matcher: a dictionary of 3-grams (last position only), no chains, no lazy evaluation"""
    seen, toks, i, n = {}, [], 0, len(data)
    while i < n:
        if i + 3 <= n:
            key = data[i:i + 3]
            j = seen.get(key)
            seen[key] = i
            if j is not None and i - j <= 32768:
                l = 3
                while l < 258 and i + l < n and data[j + l] == data[i + l]:
                    l += 1
                toks.append((l, i - j))
                i += l
                continue
        toks.append(data[i])
        i += 1
    return toks


def token_symbols(tokens):
    """(literal/length symbols incl. 256, distance symbols) a token list needs, most frequent first"""
    ll, d = {256: 1}, {}
    for t in tokens:
        if isinstance(t, (int, np.integer)):
            ll[int(t)] = ll.get(int(t), 0) + 1
        else:
            s = len_symbol(t[0], len(t) > 2 and t[2])[0]
            ll[s] = ll.get(s, 0) + 1
            s = dist_symbol(t[1])[0]
            d[s] = d.get(s, 0) + 1
    return (sorted(ll, key=lambda s: (-ll[s], s)), sorted(d, key=lambda s: (-d[s], s)))


def comb_codes_for(tokens):
    """complete codes over exactly the symbols `tokens` use, frequent symbols on the comb's short teeth, the rest as
    deep as 15 bits allow"""
    lo, do = token_symbols(tokens)
    if len(lo) < 2:
        lo.append(0 if 0 not in lo else 1)
    ll = assign(lo, deepest_comb(len(lo)), max(257, max(lo) + 1))
    if not do:
        return ll, [0]
    if len(do) == 1:
        return ll, assign(do, [1], do[0] + 1)     # the one incomplete code RFC 1951 allows
    return ll, assign(do, deepest_comb(len(do)), max(do) + 1)


def crafted_bgzf_of(data, chunk=4096):
    """[(payload, chunk bytes)]: `data` cut every `chunk` bytes regardless of its records, each piece greedy-matched and
    written as ONE dynamic block with comb codes"""
    out = []
    for o in range(0, len(data), chunk):
        piece = data[o:o + chunk]
        toks = greedy_tokens(piece)
        ll, d = comb_codes_for(toks)
        df = Deflate().dynamic(toks, ll, d, final=True)
        assert df.expected() == piece
        out.append((df, piece))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the corpora
# ---------------------------------------------------------------------------------------------------------------------
GRID_DISTS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257]
GOLD = Path(__file__).resolve().parent / "golden"


class Case:
    def __init__(self, name, df, pad=0, expected=None):
        self.name, self.df, self.blocks = name, df, df.blocks
        self.payload = df.payload(pad)
        self.expected = df.expected() if expected is None else expected
        assert len(self.expected) <= 65536 and len(self.payload) + 25 <= 65535, name


def _lits(rng, n, lo=0, hi=256):
    return [int(x) for x in rng.integers(lo, hi, n)]


def grid_tokens(rng):
    """every GRID_DISTS distance with a length below, equal to and above it (where deflate has such a length), a few
    fresh literals in front of each match so that no two sources look alike"""
    toks = _lits(rng, 300)
    for d in GRID_DISTS:
        for length in sorted({max(3, d - 1), max(3, d // 2), d, d + 1, 2 * d + 1, 258}):
            if 3 <= length <= 258:
                toks += _lits(rng, int(rng.integers(1, 4))) + [(length, d)]
    return toks


def _grow_to(rng, n):
    """tokens that produce at least n bytes cheaply: a random head, then far matches of 258"""
    toks, pos = _lits(rng, 400), 400
    while pos < n:
        toks.append((258, int(rng.integers(259, 401))))
        pos += 258
    return toks, pos


def _valid(seed=0):
    rng = np.random.default_rng(1000 + seed)
    cases = []

    def add(name, df, **kw):
        cases.append(Case(name, df, **kw))

    # ---- code lengths
    # litlen: a pure comb 1..15,15 over sixteen symbols; the length symbols and EOB sit on the long teeth
    order = [65, 66, 67, 68, 69, 70, 71, 72, 73, 257, 74, 75, 76, 285, 256, 77]
    ll = assign(order, comb_lens(16, 14), 286)
    toks = [65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77] * 3 + [(3, 1), 74, (258, 5), 75, 76, (3, 5), 77, 77, (258, 1), 65, 74]
    add("ll_codes_10_to_15_bits", Deflate().dynamic(toks, ll, assign([0, 4], [1, 1], 5), final=True))
    # distance: the same comb over sixteen distance symbols; short litlen codes in front of them
    dorder = [0, 2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 29]
    dl = assign(dorder, comb_lens(16, 14), 30)
    toks, pos = _grow_to(rng, 33000)
    toks = [t if isinstance(t, int) else (258, DIST_BASE[14] + 30) for t in toks]      # (growth by distance symbol 14 only)
    for s in dorder:
        for x in sorted({0, (1 << DIST_EXTRA[s]) - 1, int(rng.integers(0, 1 << DIST_EXTRA[s]))}):
            toks += _lits(rng, 2) + [(int(rng.integers(3, 259)), DIST_BASE[s] + x)]
    toks += [(258, 32768), 7, (3, 32768)]
    lo, _ = token_symbols(toks)
    add("dist_codes_9_to_15_bits", Deflate().dynamic(toks, assign(lo, deepest_comb(len(lo)), 286), dl, final=True))   # (symbol 285: one bit)
    # all 286 + 30 symbols present and used: every literal, every length 3..258 (258 both ways), every distance symbol
    toks = list(range(256)) + _lits(rng, 44)
    for length in [int(x) for x in rng.permutation(np.arange(3, 259))]:
        toks += [int(rng.integers(0, 256)), (length, int(rng.integers(1, 300)))]
    toks += [(258, 300, True)]
    for s in range(30):
        toks += [int(rng.integers(0, 256)), (int(rng.integers(3, 259)), DIST_BASE[s] + int(rng.integers(0, 1 << DIST_EXTRA[s])))]
    lo, do = token_symbols(toks)
    assert len(lo) == 286 and len(do) == 30
    add("all_286_and_30_symbols", Deflate().dynamic(toks, assign(lo, comb_lens(286, 6), 286), assign(do, comb_lens(30, 10), 30), final=True))
    add("every_length_fixed", Deflate().fixed(toks, final=True))
    # EOB plus one literal; no distance code at all (HDIST = 1, length 0)
    add("eob_plus_one_literal", Deflate().dynamic([33] * 777, assign([33, 256], [1, 1], 257), [0], final=True))
    toks = _lits(rng, 3000, 60, 90)
    lo, _ = token_symbols(toks)
    add("literal_only_dynamic", Deflate().dynamic(toks, assign(lo, deepest_comb(len(lo)), 257), [0], final=True))
    # one distance code of length 1
    toks = _lits(rng, 20) + [(100, 1), 9, 8, (258, 1), 7, (3, 1)]
    lo, _ = token_symbols(toks)
    add("one_distance_code_of_length_1", Deflate().dynamic(toks, assign(lo, complete_lens(len(lo)), 286), [1], final=True))

    # ---- dynamic headers
    # 16 as the first code of the distance part: it repeats the LAST LITLEN length (litlen 4 x 2 bits, the last of them
    # at the alphabet's end; distance 4 x 2 bits)
    ll = assign([65, 256, 257, 265], [2, 2, 2, 2], 266)
    hdr = [(18, 65), 2, (18, 138), (18, 52), 2, 2, (17, 7), 2, (16, 4)]
    add("hdr_16_carries_litlen_length", Deflate().dynamic([65, 65, 65, 65, (3, 1), (11, 2), 65, (12, 4), (3, 3)], ll, [2, 2, 2, 2], final=True, header=hdr))
    # an 18-run of zeros across the litlen / distance boundary; 17 at 3 and 10; 18 at 11 and 138; chained 16s at 6
    ll = [0] * 286
    for s in range(13):
        ll[s] = 4           # 13 x 4 bits
    ll[16], ll[30], ll[256] = 4, 4, 4       # 16 x 4 bits: complete
    dl = [0] * 5 + [1, 1]
    hdr = [4, (16, 6), (16, 6), (17, 3), 4, (17, 10), (17, 3), 4, (18, 138), (18, 11), (18, 76), 4, (18, 34), 1, 1]
    add("hdr_runs_17_18_16_and_boundary", Deflate().dynamic([0, 1, 2, 12, 16, 30, 5, 5], ll, dl, final=True, header=hdr))
    # the smallest HCLEN: only 16, 17, 18, 0 and 8 have a code-length code -> HCLEN = 5
    ll = [0] + [8] * 256
    add("hdr_smallest_hclen", Deflate().dynamic(_lits(rng, 500, 1, 256), ll, [0], final=True,
                                                header=[0, 8] + [(16, 6)] * 42 + [(16, 3), 0]))

    # ---- matches
    toks = grid_tokens(rng)
    add("match_grid_fixed", Deflate().fixed(toks, final=True))
    ll, dl = comb_codes_for(toks)
    add("match_grid_dynamic", Deflate().dynamic(toks, ll, dl, final=True))
    # sources that start at byte 0 of the block's output, from every small position, and runs in the first 16 bytes
    for p in (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 33, 64):
        add(f"match_source_at_byte_0_pos_{p}", Deflate().fixed(_lits(rng, p) + [(min(258, 3 * p + 2), p), 1, (3, p + 3 + min(258, 3 * p + 2) - 2)], final=True))
    add("match_ends_at_isize", Deflate().fixed(_lits(rng, 70) + [(258, 64)], final=True))
    add("match_run_ends_at_isize", Deflate().fixed(_lits(rng, 20) + [(200, 2)], final=True))
    # a source in the previous deflate block of the same BGZF block
    a, b = _lits(rng, 120), _lits(rng, 50)
    add("match_into_previous_block", Deflate().fixed(a).stored(bytes(b)).fixed([(100, 170), (50, 50), 3, (258, 9)])
        .dynamic([(30, 400), 4, (3, 1)], *comb_codes_for([(30, 400), 4, (3, 1)]), final=True))
    toks = []
    for n in (255, 256, 600):
        toks += _lits(rng, n) + [(40, n)]
    add("literal_runs_255_256_600", Deflate().fixed(toks, final=True))
    ll, dl = comb_codes_for(toks)
    add("literal_runs_255_256_600_dynamic", Deflate().dynamic(toks, ll, dl, final=True))
    toks, pos = _grow_to(rng, 32768)
    toks += [(3, 32768), 5, (258, 32768), (258, 32768, True), 6, (100, 32767)]
    add("distance_32768_fixed", Deflate().fixed(toks, final=True))

    # ---- block structure
    df = Deflate()
    for n9 in range(8):     # a fixed block of n9 nine-bit literals ends 2 + n9 bits into a byte
        df.fixed([200 + n9] * n9 + [n9]).stored(b"")
    add("empty_stored_at_every_bit_phase", df.fixed([1, 2, 3], final=True))
    add("empty_fixed_blocks_not_final", Deflate().fixed([]).fixed([]).fixed([7, 7, 7]).fixed([]).stored(b"xyz").fixed([]).fixed([(5, 2)], final=True))
    # (ISIZE 0: the host inflater decodes these; the DEVICE paths do not decode a block that claims no output at all --
    #  csrc/inflate_wave.h and csrc/inflate_kernels.h skip it, the CRC kernel compares the trailer's CRC with 0 -- so there
    #  these two check the framing and the neighbours' offsets, not a decoder)
    add("isize_0_empty_fixed", Deflate().fixed([], final=True))
    add("isize_0_empty_stored", Deflate().stored(b"", final=True))
    df, pos = Deflate(), 0
    for i in range(300):
        toks = _lits(rng, 40, 30 + i % 50, 60 + i % 50 + i % 70)
        n = 40
        while n < 160:
            d = int(rng.integers(1, min(pos + n, 3000) + 1))
            l = int(rng.integers(3, 60))
            toks += [(l, d), int(rng.integers(0, 256))]
            n += l + 1
        pos += n
        df.dynamic(toks, *comb_codes_for(toks), final=i == 299)
    add("300_dynamic_blocks", df)
    df = Deflate().fixed([1, 2, 3, (5, 3)], final=True)
    assert df.w.bitpos % 8
    add("nonzero_padding_behind_final_eob", df, pad=1)

    # ---- more sequences than the wave path's arena has room for: it must hand the block back
    add("arena_distance_9", Deflate().fixed(_lits(rng, 9) + [(3, 9)] * 21842, final=True))
    add("arena_distance_3", Deflate().fixed(_lits(rng, 3) + [(3, 3)] * 21844, final=True))

    # ---- a record stream: the golden BAM's records under comb codes, cut every 4 KiB
    for i, (df, piece) in enumerate(crafted_bgzf_of(record_stream())):
        add(f"setA_records_{i:02d}", df)
    return cases


def record_stream():
    """the inflated bytes of tests/golden/setA.bam"""
    raw, out, p = (GOLD / "setA.bam").read_bytes(), bytearray(), 0
    while p < len(raw):
        bsize = int.from_bytes(raw[p + 16:p + 18], "little") + 1
        out += zlib.decompress(raw[p + 18:p + bsize - 8], -15)
        p += bsize
    return bytes(out)


def crafted_setA_bgzf():
    """setA.bam re-compressed by this writer (BGZF blocks of 4 KiB inflated, records crossing them) + the EOF block"""
    return b"".join(bgzf_frame(df.payload(), piece) for df, piece in crafted_bgzf_of(record_stream())) + \
        bgzf_frame(Deflate().fixed([], final=True).payload(), b"")


ARENA_CASES = ("arena_distance_9", "arena_distance_3")
_CACHE = {}


def valid_case_objects(seed=0):
    if seed not in _CACHE:
        _CACHE[seed] = _valid(seed)
    return _CACHE[seed]


def valid_cases(seed=0):
    """[(name, raw deflate payload, the bytes it inflates to)]"""
    return [(c.name, c.payload, c.expected) for c in valid_case_objects(seed)]


# A decoder of this project may accept these (zlib does not): the code is incomplete, but no bit pattern of the stream
# falls into the hole, so what comes out is what the writer meant, and a stream that DID fall into the hole is refused
# (incomplete_*_hole_used).  Only over-subscription can send a canonical decoder out of its tables.
LENIENT = {
    "incomplete_litlen_set": "incomplete literal/length code whose missing codes never occur: decodes to the writer's bytes",
    "incomplete_distance_set_two_codes": "incomplete two-code distance set whose missing codes never occur: decodes to the writer's bytes",
}


class BadCase:
    """a malformed stream: .intended is what the writer meant, for the LENIENT cases only (None otherwise)"""

    def __init__(self, name, payload, isize, intended=None):
        self.name, self.payload, self.isize, self.intended = name, payload, isize, intended


def _invalid(seed=0):
    rng = np.random.default_rng(2000 + seed)
    out = []

    def add(name, df, isize, cut=None):
        p = df.payload()
        intended = bytes(replay([t for b in df.blocks for t in b["tokens"]])) if name in LENIENT else None
        out.append(BadCase(name, p if cut is None else p[:cut], isize, intended))

    for pos in (0, 1, 100):
        for by in (1, 100):
            df = Deflate()
            df.fixed(_lits(rng, pos) + [(20, pos + by)] + _lits(rng, 30), final=True)
            add(f"distance_{by}_beyond_output_at_{pos}", df, pos + 50)
    # ... the same from a dynamic block with a long distance code, and in a later deflate block of the BGZF block
    toks = _lits(rng, 40) + [(5, 7), (9, 300)]
    lo, _ = token_symbols(toks)
    add("distance_beyond_output_dynamic", Deflate().dynamic(toks, assign(lo, complete_lens(len(lo)), 286),
                                                            assign([0, 5, 2, 3, 7, 9, 11, 12, 13, 14, 16], comb_lens(11, 9), 30), final=True), 54)
    add("distance_beyond_output_second_block", Deflate().fixed(_lits(rng, 10)).stored(b"abc").fixed([(3, 14), 1], final=True), 17)
    add("output_past_isize_by_literal", Deflate().fixed(_lits(rng, 101), final=True), 100)
    add("output_past_isize_by_match", Deflate().fixed(_lits(rng, 80) + [(21, 70)], final=True), 100)
    add("output_past_isize_by_run", Deflate().fixed(_lits(rng, 80) + [(21, 1)], final=True), 100)
    add("output_past_isize_by_stored", Deflate().fixed(_lits(rng, 80)).stored(bytes(21), final=True), 100)
    add("output_short_of_isize", Deflate().fixed(_lits(rng, 80) + [(19, 70)], final=True), 100)
    for s in (286, 287):
        add(f"litlen_symbol_{s}", Deflate().fixed(_lits(rng, 10) + [("sym", s)] + _lits(rng, 10), final=True), 23)
    for s in (30, 31):
        add(f"distance_symbol_{s}", Deflate().fixed(_lits(rng, 10) + [("dsym", 3, s)] + _lits(rng, 10), final=True), 23)
    lits = _lits(rng, 30, 65, 67)
    # over-subscribed sets (three codes of one bit; for the code-length code: three of one bit)
    add("oversubscribed_litlen_set", Deflate().dynamic(lits, assign([65, 66, 256], [1, 1, 1], 257), [1, 1], final=True, strict=False), 30)
    add("oversubscribed_litlen_set_deep", Deflate().dynamic(lits, [8] * 257, [1, 1], final=True, strict=False), 30)
    add("oversubscribed_distance_set", Deflate().dynamic(lits + [(3, 1)], assign([65, 66, 256, 257], [2, 2, 2, 2], 258), [1, 1, 1], final=True, strict=False), 33)
    add("oversubscribed_code_length_set", Deflate().dynamic(lits, assign([65, 66, 256, 257], [2, 2, 2, 2], 258), [1, 1], final=True, strict=False,
                                                            cl_lens=assign([0, 1, 2], [1, 1, 1], 19)), 30)
    # incomplete sets
    add("incomplete_litlen_set", Deflate().dynamic(lits, assign([65, 66, 256], [1, 2, 3], 257), [1, 1], final=True, strict=False), 30)
    add("incomplete_litlen_hole_used", Deflate().dynamic(lits[:10] + [("bits", 7, 3)] + lits[10:], assign([65, 66, 256], [1, 2, 3], 257),
                                                         [1, 1], final=True, strict=False), 30)     # codes 0, 10, 110: 111 is none
    toks = lits + [(3, 1), 65, (4, 2)]
    add("incomplete_distance_set_two_codes", Deflate().dynamic(toks, assign([65, 66, 256, 257, 258], [2, 2, 2, 3, 3], 259), [2, 2], final=True, strict=False), 38)
    add("incomplete_distance_hole_used", Deflate().dynamic(lits + [("sym", 257), ("bits", 3, 2)] + lits, assign([65, 66, 256, 257, 258], [2, 2, 2, 3, 3], 259),
                                                           [2, 2], final=True, strict=False), 63)          # codes 00, 01: 11 is none
    # header grammar
    ll = assign([65, 66, 256, 257], [2, 2, 2, 2], 258)
    add("header_starts_with_16", Deflate().dynamic(lits, ll, [1, 1], final=True, strict=False, header=[(16, 3)] + ll[3:] + [1, 1]), 30)
    add("header_repeat_past_the_end", Deflate().dynamic(lits, ll, [1, 1], final=True, strict=False, header=ll + [1, (16, 3)]), 30)
    add("header_zero_run_past_the_end", Deflate().dynamic(lits, ll, [1, 1], final=True, strict=False, header=ll + [1, (18, 11)]), 30)
    add("no_code_for_symbol_256", Deflate().dynamic(lits, assign([65, 66], [1, 1], 257), [1, 1], final=True, strict=False, eob=False), 30)
    add("hlit_above_286", Deflate().dynamic(lits, ll + [0] * 30, [1, 1], final=True, strict=False), 30)
    # stored blocks
    add("stored_len_nlen_mismatch", Deflate().stored(b"0123456789", final=True, nlen=0x1234), 10)
    add("stored_len_past_payload", Deflate().stored(b"0123456789", final=True, length=4000), 4000)
    df = Deflate().fixed(_lits(rng, 5))
    at = df.w.bitpos            # the second block's header: BFINAL at `at`, BTYPE at at + 1 and at + 2
    p = bytearray(df.fixed(_lits(rng, 5)).payload())
    p[(at + 1) >> 3] |= 1 << ((at + 1) & 7)
    p[(at + 2) >> 3] |= 1 << ((at + 2) & 7)
    out.append(BadCase("btype_3", bytes(p), 10))
    # truncation
    df = Deflate().fixed(_lits(rng, 200, 144, 256) + [(258, 150, True)], final=True)
    n = len(df.payload())
    add("ends_in_mid_token", df, 458, cut=n - 2)       # 284 + 5 + 5 + 6 bits of match, 7 of EOB: two bytes cut into the match
    add("ends_in_mid_literals", df, 458, cut=n // 2)
    add("ends_without_final_block", Deflate().fixed(_lits(rng, 40)).fixed(_lits(rng, 40)), 80)
    return out


def invalid_case_objects(seed=0):
    if ("invalid", seed) not in _CACHE:
        _CACHE["invalid", seed] = _invalid(seed)
    return _CACHE["invalid", seed]


def invalid_cases(seed=0):
    """[(name, raw deflate payload, ISIZE the BGZF trailer should claim)] -- each malformed in ONE way.  ISIZE is never 0
    (a block that claims no output is not decoded at all)."""
    return [(c.name, c.payload, c.isize) for c in invalid_case_objects(seed)]

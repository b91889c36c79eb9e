// pss-bam_amd/csrc/deflate_kernels.h -- BGZF deflate on the device (pssbam_engine_set_block_sink, pss-bam -O ... -Z,
// pssbam_bgzf_deflate_device / _host): a byte stream in device memory becomes whole BGZF blocks, packed back to back.
//
//   bgzf_deflate    one workgroup per payload.  The stream is cut at FIXED offsets: payload k is bytes [k * 0xFF00,
//                   min((k + 1) * 0xFF00, total)), whatever the record boundaries are (as htsjdk cuts).  The
//                   workgroup writes the complete block (18-byte header with the BC field, raw DEFLATE, CRC-32, ISIZE) at
//                   comp + k * 65536 and its length to comp_len[k].  One DEFLATE block per payload, BFINAL set: dynamic
//                   Huffman over LZ77 tokens, or stored when that is not smaller.
//   bgzf_pack_scan  exclusive scan of comp_len[] (one workgroup, a carry between rounds) and the totals {bytes, blocks}
//   bgzf_pack_copy  block k to its packed place, one workgroup per block
//
// The encoder (deflate_block) keeps the payload in LDS and works in segments of 1024 positions, one per thread:
//   match   a position hashes its 4 bytes into a table of "latest position with this hash".  Within a segment the waves
//           take turns in position order, and inside a wave a lane takes the nearest earlier lane with its hash: the
//           candidate of a position is the nearest earlier position with the same hash, a rule, not a race.  The candidate and
//           the position before (runs) are verified against the bytes and extended; distances <= 32768, lengths 3..258,
//           never past the payload's end.
//   parse   greedy from position 0: pointer doubling over jump[] marks the token starts of the segment, the chain's exit
//           is the next segment's start.
//   It runs twice with the same outcome: once for the histograms, and after the code lengths are built (length-limited
//   to 15, code-length code to 7; at least two codes in every alphabet) once to prefix-sum the token lengths and OR the
//   bits into a staging image that is flushed to the block a segment at a time.  The size is known after the first pass, so
//   BSIZE is written up front and stored is chosen before a byte goes out.
// Nothing depends on timing: table updates are atomicMax in a fixed order of waves, histogram adds and bit ORs commute.
//
// The per-thread state that crosses a barrier lives in LDS arrays, and the phases are written with DFL_FOR_THREADS /
// DFL_END_THREADS: compiled with DFL_EMULATE for the host, a phase is a loop over the threads, and the encoder can be run
// and checked without a device.
#pragma once

#include <stdint.h>

#ifdef DFL_EMULATE
#define DFL_FN static inline
#define DFL_FOR_THREADS for (uint32_t tid = 0; tid < DFL_THREADS; tid++) {
#define DFL_END_THREADS }
static inline uint32_t dfl_atomic_max(uint32_t *p, uint32_t v) { const uint32_t o = *p; if (v > o) *p = v; return o; }
static inline uint32_t dfl_atomic_add(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
static inline uint32_t dfl_atomic_or(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o | v; return o; }
static inline uint32_t dfl_atomic_xor(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o ^ v; return o; }
static inline uint32_t dfl_brev(uint32_t v) { uint32_t r = 0; for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i); return r; }
static inline uint32_t dfl_ctz(uint32_t v) { return (uint32_t)__builtin_ctz(v); }
static inline uint32_t dfl_clz(uint32_t v) { return (uint32_t)__builtin_clz(v); }
static inline uint32_t dfl_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * sh)); }
#else
#define DFL_FN __device__ __forceinline__
#define DFL_FOR_THREADS { const uint32_t tid = threadIdx.x;
#define DFL_END_THREADS } __syncthreads();
#define dfl_atomic_max atomicMax
#define dfl_atomic_add atomicAdd
#define dfl_atomic_or atomicOr
#define dfl_atomic_xor atomicXor
#define dfl_brev __brev
DFL_FN uint32_t dfl_ctz(uint32_t v) { return (uint32_t)__builtin_ctz(v); }
DFL_FN uint32_t dfl_clz(uint32_t v) { return (uint32_t)__builtin_clz(v); }
#define dfl_alignbyte __builtin_amdgcn_alignbyte
#endif

namespace pssbam {

constexpr uint32_t DFL_PAYLOAD = 0xFF00u;       // bytes of the stream per BGZF block
constexpr uint32_t DFL_SLOT = 65536u;           // a block's place in the strided buffer: the largest BGZF block
constexpr uint32_t DFL_THREADS = 1024u;         // = positions per segment
constexpr uint32_t DFL_HASH_BITS = 14u;
constexpr uint32_t DFL_NO_HASH = 0xFFFFu;
constexpr uint32_t DFL_STORED_EXTRA = 5u + 26u; // stored: 1 + LEN + NLEN; BGZF: 18 + 8
constexpr uint32_t DFL_STAGE_WORDS = 1024u + 8u;
constexpr uint32_t DFL_CRC_CHUNK = 64u;         // bytes per thread of the CRC; xpow64[k] = x^(8 * 64 * k) mod P
constexpr uint32_t DFL_CRC_POLY = 0xEDB88320u;

struct alignas(16) DflQuad { uint32_t v[4]; };

struct DeflateShared {
    uint32_t data[DFL_SLOT / 4 + 4];            // the payload, zeros behind it
    uint32_t table[1u << DFL_HASH_BITS];        // 1 + the latest position with this hash; 0: none
    uint16_t h[DFL_THREADS], len[DFL_THREADS], dist[DFL_THREADS], jump[2][DFL_THREADS], bits[DFL_THREADS];
    uint8_t mark[DFL_THREADS];
    uint32_t part[34];
    uint32_t stage[DFL_STAGE_WORDS];            // the output image from word w0 on
    uint32_t hist_ll[288], hist_d[32], hist_cl[20];
    uint8_t len_ll[288], len_d[32], len_cl[20];
    uint16_t code_ll[288], code_d[32], code_cl[20];
    uint16_t sorted[288], parent[576];
    uint32_t weight[576], bl_count[16], next_code[16];
    uint16_t clsym[320];                        // the code-length sequence: symbol | extra << 8
    uint32_t crc_tab[256];
    uint32_t n_used, n_clsym, carry, bitpos, w0, carry_word, seg_bits, crc, hlit, hdist, hclen, data_bits, dummy0, dummy1;
};

DFL_FN uint32_t dfl_load32(const DeflateShared &S, uint32_t at) {
    const uint32_t w = at >> 2, sh = at & 3u;
    const uint32_t lo = S.data[w];
    return sh ? dfl_alignbyte(S.data[w + 1], lo, sh) : lo;
}
DFL_FN uint32_t dfl_byte(const DeflateShared &S, uint32_t at) { return (S.data[at >> 2] >> (8u * (at & 3u))) & 0xFFu; }

// equal bytes at p and q (q < p), at most maxlen
DFL_FN uint32_t dfl_match_len(const DeflateShared &S, uint32_t p, uint32_t q, uint32_t maxlen) {
    uint32_t l = 0;
    while (l < maxlen) {
        const uint32_t x = dfl_load32(S, p + l) ^ dfl_load32(S, q + l);
        if (x) { l += dfl_ctz(x) >> 3; break; }
        l += 4u;
    }
    return l < maxlen ? l : maxlen;
}

// RFC 1951 3.2.5: the symbol, the number of extra bits and their value of a length (3..258) and of a distance (1..32768)
DFL_FN void dfl_len_sym(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t l = len - 3u;
    if (len == 258u) { sym = 285u; eb = 0u; ev = 0u; }
    else if (l < 8u) { sym = 257u + l; eb = 0u; ev = 0u; }
    else {
        const uint32_t k = 31u - dfl_clz(l);
        eb = k - 2u;
        sym = 261u + 4u * eb + ((l - (1u << k)) >> eb);
        ev = l & ((1u << eb) - 1u);
    }
}
DFL_FN void dfl_dist_sym(uint32_t dist, uint32_t &sym, uint32_t &eb, uint32_t &ev) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { sym = d; eb = 0u; ev = 0u; }
    else {
        const uint32_t k = 31u - dfl_clz(d);
        eb = k - 1u;
        sym = 2u * k + ((d >> (k - 1u)) & 1u);
        ev = d & ((1u << eb) - 1u);
    }
}
DFL_FN uint32_t dfl_ll_extra(uint32_t sym) { return (sym < 265u || sym == 285u) ? 0u : (sym - 261u) >> 2; }
DFL_FN uint32_t dfl_d_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }

// ORs the low nbits (<= 57) of v into the image at bit `pos`
DFL_FN void dfl_put_bits(DeflateShared &S, uint32_t pos, uint64_t v, uint32_t nbits) {
    uint32_t w = (pos >> 5) - S.w0, sh = pos & 31u;
    while (nbits) {
        const uint32_t take = nbits < 32u - sh ? nbits : 32u - sh;
        const uint32_t piece = (uint32_t)(v & ((1ull << take) - 1ull));
        if (piece) dfl_atomic_or(&S.stage[w], piece << sh);
        v >>= take;
        nbits -= take;
        w++;
        sh = 0u;
    }
}

// Code lengths of at most maxbits for the n symbols of freq[] (every thread of the workgroup calls it).  An alphabet with
// fewer than two used symbols gets one or two more with a count of one, which are taken out of freq[] again: every code is
// complete.  The lengths are those of a Huffman tree, longer ones cut to maxbits and the overflow moved up as zlib's
// gen_bitlen does, then dealt out by frequency.
DFL_FN void dfl_build_lengths(DeflateShared &S, uint32_t *freq, uint32_t n, uint32_t maxbits, uint8_t *len_out) {
    DFL_FOR_THREADS
        if (tid == 0) { S.n_used = 0u; S.dummy0 = S.dummy1 = DFL_NO_HASH; }
        if (tid < 16u) S.bl_count[tid] = 0u;
        if (tid < n) len_out[tid] = 0;
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid < n && freq[tid]) dfl_atomic_add(&S.n_used, 1u);
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid == 0 && S.n_used < 2u) {
            if (S.n_used == 0u) { freq[0] = freq[1] = 1u; S.dummy0 = 0u; S.dummy1 = 1u; }
            else {
                const uint32_t d = freq[0] ? 1u : 0u;
                freq[d] = 1u;
                S.dummy0 = d;
            }
            S.n_used = 2u;
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid < n && freq[tid]) {
            const uint32_t f = freq[tid];
            uint32_t rank = 0u;
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t g = freq[j];
                rank += (g && (g < f || (g == f && j < tid))) ? 1u : 0u;
            }
            S.sorted[rank] = (uint16_t)tid;
            S.weight[rank] = f;
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid == 0) {   // the two-queue merge: leaves [0, m) in order of weight, inner nodes [m, 2m - 1) as they are made
            const uint32_t m = S.n_used;
            uint32_t a = 0u, b = m;
            for (uint32_t next = m; next < 2u * m - 1u; next++) {
                uint32_t w = 0u;
                for (int k = 0; k < 2; k++) {
                    uint32_t pick;
                    if (a < m && (b >= next || S.weight[a] <= S.weight[b])) pick = a++;
                    else pick = b++;
                    w += S.weight[pick];
                    S.parent[pick] = (uint16_t)next;
                }
                S.weight[next] = w;
            }
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid < S.n_used) {
            const uint32_t root = 2u * S.n_used - 2u;
            uint32_t d = 0u, node = tid;
            while (node != root) { node = S.parent[node]; d++; }
            dfl_atomic_add(&S.bl_count[d < maxbits ? d : maxbits], 1u);
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid == 0) {
            uint32_t kraft = 0u;
            for (uint32_t l = 1; l <= maxbits; l++) kraft += S.bl_count[l] << (maxbits - l);
            for (uint32_t over = kraft - (1u << maxbits); over > 0u; over--) {   // each step takes exactly one off the Kraft sum
                uint32_t bits = maxbits - 1u;
                while (S.bl_count[bits] == 0u) bits--;
                S.bl_count[bits]--;
                S.bl_count[bits + 1u] += 2u;
                S.bl_count[maxbits]--;
            }
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid < S.n_used) {   // rank 0 is the rarest symbol: the longest codes first
            uint32_t cum = 0u, l = maxbits;
            for (; l > 1u; l--) {
                if (tid < cum + S.bl_count[l]) break;
                cum += S.bl_count[l];
            }
            len_out[S.sorted[tid]] = (uint8_t)l;
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid == 0) {
            if (S.dummy0 != DFL_NO_HASH) freq[S.dummy0] = 0u;
            if (S.dummy1 != DFL_NO_HASH) freq[S.dummy1] = 0u;
        }
    DFL_END_THREADS
}

// canonical codes (RFC 1951 3.2.2) of the lengths, bit-reversed: DEFLATE packs Huffman codes from their top bit
DFL_FN void dfl_build_codes(DeflateShared &S, const uint8_t *len, uint32_t n, uint16_t *code_out) {
    DFL_FOR_THREADS
        if (tid < 16u) S.bl_count[tid] = 0u;
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid < n && len[tid]) dfl_atomic_add(&S.bl_count[len[tid]], 1u);
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid == 0) {
            uint32_t code = 0u;
            S.next_code[0] = 0u;
            for (uint32_t l = 1; l < 16u; l++) {
                code = (code + S.bl_count[l - 1u]) << 1;
                S.next_code[l] = code;
            }
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        if (tid < n) {
            const uint32_t l = len[tid];
            uint32_t c = 0u;
            if (l) {
                c = S.next_code[l];
                for (uint32_t j = 0; j < tid; j++) c += len[j] == l ? 1u : 0u;
                c = dfl_brev(c) >> (32u - l);
            }
            code_out[tid] = (uint16_t)c;
        }
    DFL_END_THREADS
}

// One segment's matches and token starts: after it mark[t] says whether position seg * 1024 + t starts a token, and
// len[t] / dist[t] are its match (len 0: a literal).  Same state in, same tokens out: both passes call it.
DFL_FN void dfl_segment(DeflateShared &S, uint32_t n, uint32_t seg) {
    const uint32_t base = seg * DFL_THREADS;
    DFL_FOR_THREADS
        const uint32_t p = base + tid;
        uint32_t h = DFL_NO_HASH;
        if (p + 4u <= n) h = (dfl_load32(S, p) * 0x9E3779B1u) >> (32u - DFL_HASH_BITS);
        S.h[tid] = (uint16_t)h;
    DFL_END_THREADS
    for (uint32_t turn = 0; turn < DFL_THREADS / 64u; turn++) {
        DFL_FOR_THREADS
            if ((tid >> 6) == turn) {
                const uint32_t h = S.h[tid], p = base + tid;
                uint32_t d = 0u;
                if (h != DFL_NO_HASH) {
                    for (uint32_t j = tid & ~63u; j < tid; j++)
                        if (S.h[j] == h) d = tid - j;   // the nearest earlier lane of this wave
                    const uint32_t seen = S.table[h];     // what the waves before left: no lane of this wave if d == 0
                    dfl_atomic_max(&S.table[h], p + 1u);
                    if (!d && seen) d = p + 1u - seen;
                }
                S.dist[tid] = (uint16_t)d;
            }
        DFL_END_THREADS
    }
    DFL_FOR_THREADS
        const uint32_t p = base + tid;
        uint32_t best = 0u, bd = 0u;
        if (p < n) {
            const uint32_t maxlen = n - p < 258u ? n - p : 258u;
            const uint32_t d = S.dist[tid];
            if (d && d <= 32768u && d <= p) {
                const uint32_t l = dfl_match_len(S, p, p - d, maxlen);
                if (l >= 4u) { best = l; bd = d; }
            }
            if (p >= 1u && maxlen >= 3u) {
                const uint32_t l = dfl_match_len(S, p, p - 1u, maxlen);
                if (l >= 3u && l >= best) { best = l; bd = 1u; }
            }
        }
        S.len[tid] = (uint16_t)best;
        S.dist[tid] = (uint16_t)bd;
        S.jump[0][tid] = (uint16_t)(tid + (best ? best : 1u));
        S.mark[tid] = p == S.carry ? 1 : 0;
    DFL_END_THREADS
    if (S.carry >= base + DFL_THREADS) return;   // a match of the segment before covers all of this one
    for (uint32_t k = 0; k < 10u; k++) {
        const uint32_t src = k & 1u;
        DFL_FOR_THREADS
            const uint32_t j = S.jump[src][tid];
            if (S.mark[tid] && j < DFL_THREADS) S.mark[j] = 1;
            S.jump[src ^ 1u][tid] = j < DFL_THREADS ? S.jump[src][j] : (uint16_t)j;
        DFL_END_THREADS
    }
}

DFL_FN uint32_t dfl_crc_bytes(const DeflateShared &S, uint32_t crc, uint32_t s, uint32_t e) {
    for (uint32_t i = s; i < e; i++) crc = S.crc_tab[(crc ^ dfl_byte(S, i)) & 0xFFu] ^ (crc >> 8);
    return crc;
}
DFL_FN uint32_t dfl_gf2_mul(uint32_t a, uint32_t b) {   // as gf2_mul of inflate_kernels.h
    uint32_t r = 0u;
    for (int i = 0; i < 32; i++) {
        r ^= (b & 0x80000000u) ? a : 0u;
        b <<= 1;
        a = (a >> 1) ^ ((a & 1u) ? DFL_CRC_POLY : 0u);
    }
    return r;
}

// byte i of a stored block of the payload
DFL_FN uint32_t dfl_stored_byte(const DeflateShared &S, uint32_t i, uint32_t n, uint32_t crc) {
    const uint32_t bsize = 18u + 5u + n + 8u - 1u;
    const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    if (i < 16u) return hdr[i];
    if (i == 16u) return bsize & 0xFFu;
    if (i == 17u) return bsize >> 8;
    if (i == 18u) return 1u;   // BFINAL, BTYPE 00
    if (i == 19u) return n & 0xFFu;
    if (i == 20u) return n >> 8;
    if (i == 21u) return ~n & 0xFFu;
    if (i == 22u) return (~n >> 8) & 0xFFu;
    if (i < 23u + n) return dfl_byte(S, i - 23u);
    const uint32_t t = i - 23u - n;
    return ((t < 4u ? crc : n) >> (8u * (t & 3u))) & 0xFFu;
}

// The payload raw[0, n) (1 <= n <= 0xFF00; raw 16-byte aligned, readable up to the next multiple of 16) becomes one BGZF
// block at out (4-byte aligned, DFL_SLOT bytes); *out_len = its length.
DFL_FN void deflate_block(DeflateShared &S, const uint8_t *raw, uint32_t n, uint8_t *out, uint32_t *out_len, const uint32_t *xpow64) {
    const DflQuad *rawq = (const DflQuad *)raw;
    uint32_t *out32 = (uint32_t *)out;
    const uint32_t n_seg = (n + DFL_THREADS - 1u) / DFL_THREADS;
    DFL_FOR_THREADS
        for (uint32_t q = tid; q < DFL_SLOT / 16u + 1u; q += DFL_THREADS) {   // lane i next to lane i - 1, 16 bytes each
            DflQuad v = {{0u, 0u, 0u, 0u}};
            if (q * 16u < n) v = rawq[q];
            for (uint32_t j = 0; j < 4u; j++) {
                const uint32_t b = q * 16u + 4u * j;
                uint32_t w = v.v[j];
                if (b >= n) w = 0u;
                else if (b + 4u > n) w &= (1u << (8u * (n - b))) - 1u;
                S.data[4u * q + j] = w;
            }
        }
        for (uint32_t i = tid; i < (1u << DFL_HASH_BITS); i += DFL_THREADS) S.table[i] = 0u;
        for (uint32_t i = tid; i < DFL_STAGE_WORDS; i += DFL_THREADS) S.stage[i] = 0u;
        if (tid < 288u) S.hist_ll[tid] = 0u;
        if (tid < 32u) S.hist_d[tid] = 0u;
        if (tid < 20u) S.hist_cl[tid] = 0u;
        if (tid < 256u) {
            uint32_t c = tid;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? DFL_CRC_POLY : 0u);
            S.crc_tab[tid] = c;
        }
        if (tid == 0) { S.carry = 0u; S.crc = 0u; S.data_bits = 0u; S.n_clsym = 0u; S.w0 = 0u; }
    DFL_END_THREADS
    // CRC-32: thread c owns the 64 bytes that end 64 * c bytes before the payload's end (bgzf_crc_kernel's scheme)
    DFL_FOR_THREADS
        const uint32_t behind = tid * DFL_CRC_CHUNK;
        const uint32_t e = n > behind ? n - behind : 0u, s = e > DFL_CRC_CHUNK ? e - DFL_CRC_CHUNK : 0u;
        if (e > 0u) {
            uint32_t crc = dfl_crc_bytes(S, s == 0u ? 0xFFFFFFFFu : 0u, s, e);
            if (behind) crc = dfl_gf2_mul(crc, xpow64[tid]);
            dfl_atomic_xor(&S.crc, crc);
        }
    DFL_END_THREADS
    const uint32_t crc = ~S.crc;

    // pass 1: the histograms
    for (uint32_t seg = 0; seg < n_seg; seg++) {
        dfl_segment(S, n, seg);
        DFL_FOR_THREADS
            const uint32_t p = seg * DFL_THREADS + tid;
            if (S.mark[tid] && p < n) {
                const uint32_t l = S.len[tid];
                if (l) {
                    uint32_t sym, eb, ev;
                    dfl_len_sym(l, sym, eb, ev);
                    dfl_atomic_add(&S.hist_ll[sym], 1u);
                    dfl_dist_sym(S.dist[tid], sym, eb, ev);
                    dfl_atomic_add(&S.hist_d[sym], 1u);
                } else {
                    dfl_atomic_add(&S.hist_ll[dfl_byte(S, p)], 1u);
                }
                if (tid + (l ? l : 1u) >= DFL_THREADS) S.carry = p + (l ? l : 1u);
            }
        DFL_END_THREADS
    }
    DFL_FOR_THREADS
        if (tid == 0) S.hist_ll[256] = 1u;
    DFL_END_THREADS
    dfl_build_lengths(S, S.hist_ll, 286u, 15u, S.len_ll);
    dfl_build_lengths(S, S.hist_d, 30u, 15u, S.len_d);
    dfl_build_codes(S, S.len_ll, 286u, S.code_ll);
    dfl_build_codes(S, S.len_d, 30u, S.code_d);
    // the code lengths as the header carries them: runs as symbols 16, 17, 18
    DFL_FOR_THREADS
        if (tid == 0) {
            uint32_t hlit = 286u, hdist = 30u;
            while (hlit > 257u && !S.len_ll[hlit - 1u]) hlit--;
            while (hdist > 1u && !S.len_d[hdist - 1u]) hdist--;
            S.hlit = hlit;
            S.hdist = hdist;
            const uint32_t total = hlit + hdist;
            uint32_t m = 0u;
#define DFL_L(i) ((i) < hlit ? S.len_ll[(i)] : S.len_d[(i) - hlit])
#define DFL_EMIT(sym, extra) do { S.clsym[m++] = (uint16_t)((sym) | ((extra) << 8)); S.hist_cl[(sym)]++; } while (0)
            for (uint32_t i = 0; i < total;) {
                const uint32_t v = DFL_L(i);
                uint32_t run = 1u;
                while (i + run < total && DFL_L(i + run) == v) run++;
                uint32_t rem = run;
                if (v == 0u) {
                    while (rem >= 11u) { const uint32_t r = rem < 138u ? rem : 138u; DFL_EMIT(18u, r - 11u); rem -= r; }
                    if (rem >= 3u) { DFL_EMIT(17u, rem - 3u); rem = 0u; }
                    for (; rem > 0u; rem--) DFL_EMIT(0u, 0u);
                } else {
                    DFL_EMIT(v, 0u);
                    rem--;
                    while (rem >= 3u) { const uint32_t r = rem < 6u ? rem : 6u; DFL_EMIT(16u, r - 3u); rem -= r; }
                    for (; rem > 0u; rem--) DFL_EMIT(v, 0u);
                }
                i += run;
            }
#undef DFL_EMIT
#undef DFL_L
            S.n_clsym = m;
        }
    DFL_END_THREADS
    dfl_build_lengths(S, S.hist_cl, 19u, 7u, S.len_cl);
    dfl_build_codes(S, S.len_cl, 19u, S.code_cl);
    DFL_FOR_THREADS
        if (tid < 286u && S.hist_ll[tid]) dfl_atomic_add(&S.data_bits, S.hist_ll[tid] * (S.len_ll[tid] + dfl_ll_extra(tid)));
        if (tid < 30u && S.hist_d[tid]) dfl_atomic_add(&S.data_bits, S.hist_d[tid] * (S.len_d[tid] + dfl_d_extra(tid)));
        if (tid < 19u && S.hist_cl[tid]) dfl_atomic_add(&S.data_bits, S.hist_cl[tid] * (S.len_cl[tid] + (tid == 16u ? 2u : tid == 17u ? 3u : tid == 18u ? 7u : 0u)));
        if (tid == 0) {
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            uint32_t hclen = 19u;
            while (hclen > 4u && !S.len_cl[order[hclen - 1u]]) hclen--;
            S.hclen = hclen;
        }
    DFL_END_THREADS
    const uint32_t deflate_bits = 3u + 5u + 5u + 4u + 3u * S.hclen + S.data_bits;
    const uint32_t dyn_total = 18u + (deflate_bits + 7u) / 8u + 8u, stored_total = 18u + 5u + n + 8u;
    if (dyn_total >= stored_total) {
        DFL_FOR_THREADS
            for (uint32_t i = tid; i < stored_total; i += DFL_THREADS) out[i] = (uint8_t)dfl_stored_byte(S, i, n, crc);
            if (tid == 0) *out_len = stored_total;
        DFL_END_THREADS
        return;
    }

    // pass 2: the same tokens again, now written
    DFL_FOR_THREADS
        for (uint32_t i = tid; i < (1u << DFL_HASH_BITS); i += DFL_THREADS) S.table[i] = 0u;
        if (tid == 0) {
            const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
            S.carry = 0u;
            S.stage[0] = 0x04088b1fu;
            S.stage[1] = 0u;
            S.stage[2] = 0x0006ff00u;
            S.stage[3] = 0x00024342u;
            S.stage[4] = dyn_total - 1u;   // BSIZE
            uint32_t pos = 144u;
            dfl_put_bits(S, pos, 1u | (2u << 1), 3u); pos += 3u;
            dfl_put_bits(S, pos, S.hlit - 257u, 5u); pos += 5u;
            dfl_put_bits(S, pos, S.hdist - 1u, 5u); pos += 5u;
            dfl_put_bits(S, pos, S.hclen - 4u, 4u); pos += 4u;
            for (uint32_t i = 0; i < S.hclen; i++) { dfl_put_bits(S, pos, S.len_cl[order[i]], 3u); pos += 3u; }
            for (uint32_t i = 0; i < S.n_clsym; i++) {
                const uint32_t sym = S.clsym[i] & 0xFFu, extra = S.clsym[i] >> 8;
                dfl_put_bits(S, pos, S.code_cl[sym], S.len_cl[sym]); pos += S.len_cl[sym];
                const uint32_t eb = sym == 16u ? 2u : sym == 17u ? 3u : sym == 18u ? 7u : 0u;
                if (eb) { dfl_put_bits(S, pos, extra, eb); pos += eb; }
            }
            S.bitpos = pos;
        }
    DFL_END_THREADS
    for (uint32_t seg = 0; seg < n_seg; seg++) {
        dfl_segment(S, n, seg);
        DFL_FOR_THREADS
            const uint32_t p = seg * DFL_THREADS + tid;
            uint32_t bits = 0u;
            if (S.mark[tid] && p < n) {
                const uint32_t l = S.len[tid];
                if (l) {
                    uint32_t sym, eb, ev;
                    dfl_len_sym(l, sym, eb, ev);
                    bits = S.len_ll[sym] + eb;
                    dfl_dist_sym(S.dist[tid], sym, eb, ev);
                    bits += S.len_d[sym] + eb;
                } else {
                    bits = S.len_ll[dfl_byte(S, p)];
                }
                if (tid + (l ? l : 1u) >= DFL_THREADS) S.carry = p + (l ? l : 1u);
            }
            S.bits[tid] = (uint16_t)bits;
        DFL_END_THREADS
        // exclusive prefix sum of bits[]: 32 runs of 32
        DFL_FOR_THREADS
            if (tid < 32u) {
                uint32_t s = 0u;
                for (uint32_t j = 0; j < 32u; j++) s += S.bits[tid * 32u + j];
                S.part[tid] = s;
            }
        DFL_END_THREADS
        DFL_FOR_THREADS
            if (tid == 0) {
                uint32_t s = 0u;
                for (uint32_t j = 0; j < 32u; j++) { const uint32_t v = S.part[j]; S.part[j] = s; s += v; }
                S.seg_bits = s;
            }
        DFL_END_THREADS
        DFL_FOR_THREADS
            const uint32_t bits = S.bits[tid];
            if (bits) {
                uint32_t pos = S.bitpos + S.part[tid >> 5];
                for (uint32_t j = tid & ~31u; j < tid; j++) pos += S.bits[j];
                const uint32_t l = S.len[tid];
                if (l) {
                    uint32_t sym, eb, ev, sh;
                    dfl_len_sym(l, sym, eb, ev);
                    uint64_t v = S.code_ll[sym];
                    sh = S.len_ll[sym];
                    v |= (uint64_t)ev << sh;
                    sh += eb;
                    dfl_dist_sym(S.dist[tid], sym, eb, ev);
                    v |= (uint64_t)S.code_d[sym] << sh;
                    sh += S.len_d[sym];
                    v |= (uint64_t)ev << sh;
                    dfl_put_bits(S, pos, v, bits);
                } else {
                    dfl_put_bits(S, pos, S.code_ll[dfl_byte(S, seg * DFL_THREADS + tid)], bits);
                }
            }
        DFL_END_THREADS
        // the whole words of the image go out; the word the next token starts in stays
        DFL_FOR_THREADS
            const uint32_t n_words = ((S.bitpos + S.seg_bits) >> 5) - S.w0;
            for (uint32_t i = tid; i < n_words; i += DFL_THREADS) out32[S.w0 + i] = S.stage[i];
            if (tid == 0) S.carry_word = S.stage[n_words];
        DFL_END_THREADS
        DFL_FOR_THREADS
            for (uint32_t i = tid; i < DFL_STAGE_WORDS; i += DFL_THREADS) S.stage[i] = i ? 0u : S.carry_word;
        DFL_END_THREADS
        DFL_FOR_THREADS
            if (tid == 0) {
                const uint32_t end = S.bitpos + S.seg_bits;
                S.w0 = end >> 5;
                S.bitpos = end;
            }
        DFL_END_THREADS
    }
    DFL_FOR_THREADS
        if (tid == 0) {   // end of block, up to the byte, CRC-32, ISIZE
            uint32_t pos = S.bitpos;
            dfl_put_bits(S, pos, S.code_ll[256], S.len_ll[256]);
            pos = (pos + S.len_ll[256] + 7u) & ~7u;
            dfl_put_bits(S, pos, crc, 32u);
            dfl_put_bits(S, pos + 32u, n, 32u);
            S.bitpos = pos + 64u;
        }
    DFL_END_THREADS
    DFL_FOR_THREADS
        const uint32_t n_words = ((S.bitpos + 31u) >> 5) - S.w0;
        for (uint32_t i = tid; i < n_words; i += DFL_THREADS) out32[S.w0 + i] = S.stage[i];
        if (tid == 0) *out_len = S.bitpos >> 3;
    DFL_END_THREADS
}

#ifndef DFL_EMULATE
// total_ptr != NULL: the stream's length is read from device memory (what select_scan_sums wrote); the grid is sized for the
// host's bound of it and a workgroup whose payload does not exist leaves
__global__ void __launch_bounds__(DFL_THREADS) bgzf_deflate(const uint8_t *raw, const unsigned long long *total_ptr, unsigned long long total_imm,
                                                            uint8_t *comp, uint32_t *comp_len, const uint32_t *xpow64) {
    __shared__ DeflateShared S;
    const unsigned long long total = total_ptr ? *total_ptr : total_imm;
    const unsigned long long n_blocks = (total + DFL_PAYLOAD - 1ull) / DFL_PAYLOAD;
    for (unsigned long long k = blockIdx.x; k < n_blocks; k += gridDim.x) {
        const unsigned long long at = k * DFL_PAYLOAD;
        const uint32_t n = (uint32_t)(total - at < DFL_PAYLOAD ? total - at : DFL_PAYLOAD);
        deflate_block(S, raw + at, n, comp + k * DFL_SLOT, comp_len + k, xpow64);
        __syncthreads();
    }
}

constexpr uint32_t PACK_SCAN_THREADS = 64;   // block lengths per round

// off[k] = where block k goes; totals_out = {bytes, blocks}
__global__ void __launch_bounds__(PACK_SCAN_THREADS) bgzf_pack_scan(const uint32_t *comp_len, const unsigned long long *total_ptr, unsigned long long total_imm,
                                                                    unsigned long long *off, unsigned long long *totals_out) {
    __shared__ unsigned long long lds[2][PACK_SCAN_THREADS];
    const unsigned long long total = total_ptr ? *total_ptr : total_imm;
    const unsigned long long n_blocks = (total + DFL_PAYLOAD - 1ull) / DFL_PAYLOAD;
    unsigned long long carry = 0ull;
    for (unsigned long long k0 = 0; k0 < n_blocks; k0 += PACK_SCAN_THREADS) {
        const unsigned long long k = k0 + threadIdx.x;
        const unsigned long long mine = k < n_blocks ? comp_len[k] : 0ull;
        uint32_t cur = 0u;
        lds[0][threadIdx.x] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < PACK_SCAN_THREADS; d <<= 1) {
            unsigned long long v = lds[cur][threadIdx.x];
            if (threadIdx.x >= d) v += lds[cur][threadIdx.x - d];
            lds[cur ^ 1u][threadIdx.x] = v;
            cur ^= 1u;
            __syncthreads();
        }
        if (k < n_blocks) off[k] = carry + lds[cur][threadIdx.x] - mine;
        carry += lds[cur][PACK_SCAN_THREADS - 1u];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        totals_out[0] = carry;
        totals_out[1] = n_blocks;
    }
}

constexpr uint32_t PACK_COPY_THREADS = 256;

// block k from its slot (16-byte aligned) to out + off[k] (any alignment): bytes up to the destination's next 16-byte
// boundary, then 16 bytes a lane built from aligned dwords of the source, then the bytes that are left
__global__ void __launch_bounds__(PACK_COPY_THREADS) bgzf_pack_copy(const uint8_t *comp, const uint32_t *comp_len, const unsigned long long *off,
                                                                    const unsigned long long *total_ptr, unsigned long long total_imm, uint8_t *out) {
    const unsigned long long total = total_ptr ? *total_ptr : total_imm;
    const unsigned long long n_blocks = (total + DFL_PAYLOAD - 1ull) / DFL_PAYLOAD;
    for (unsigned long long k = blockIdx.x; k < n_blocks; k += gridDim.x) {
        const uint8_t *src = comp + k * DFL_SLOT;
        uint8_t *dst = out + off[k];
        const uint32_t len = comp_len[k];
        uint32_t lead = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);
        if (lead > len) lead = len;
        const uint32_t n_quads = (len - lead) / 16u, tail = lead + n_quads * 16u;
        if (threadIdx.x < lead) dst[threadIdx.x] = src[threadIdx.x];
        const uint32_t sh = lead & 3u;
        for (uint32_t q = threadIdx.x; q < n_quads; q += PACK_COPY_THREADS) {
            const uint32_t at = lead + q * 16u;
            const uint32_t *s = (const uint32_t *)(src + (at & ~3u));
            DflQuad v;
            if (sh) {   // (the fifth dword holds a byte of the block: at + 16 <= len - 1 or it is not read)
                const uint32_t a = s[0], b = s[1], c = s[2], d = s[3];
                const uint32_t e = (at & ~3u) + 16u < len ? s[4] : 0u;
                v.v[0] = __builtin_amdgcn_alignbyte(b, a, sh);
                v.v[1] = __builtin_amdgcn_alignbyte(c, b, sh);
                v.v[2] = __builtin_amdgcn_alignbyte(d, c, sh);
                v.v[3] = __builtin_amdgcn_alignbyte(e, d, sh);
            } else {
                v.v[0] = s[0]; v.v[1] = s[1]; v.v[2] = s[2]; v.v[3] = s[3];
            }
            *(DflQuad *)(dst + at) = v;
        }
        if (threadIdx.x < len - tail) dst[tail + threadIdx.x] = src[tail + threadIdx.x];
    }
}
#endif

}  // namespace pssbam

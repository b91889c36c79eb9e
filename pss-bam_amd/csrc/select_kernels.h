// pss-bam_amd/csrc/select_kernels.h -- the record sink's device path (pssbam_engine_set_record_sink, pss-bam -O): which
// records of a block were added to the forward or the reverse main table, and those records, byte for byte and in input
// order, in one contiguous buffer.  Three steps behind the tally kernels of the same block, on the same stream:
//
//   select_mark    lane per read: the decision of tally_simple (decode_hdr, make_plan in its GAPPED form under -I, the -n
//                  and -y filters: select_keep, which coverage_kernels.h asks too), written as len[r] = kept ? record length : 0.
//                  No counter, no event, no table add.
//   scan           exclusive prefix sum of len[] in place, plus the totals {bytes, records} kept: select_tile_sums (a sum
//                  pair per tile of SELECT_SCAN_TILE entries), select_scan_sums (one workgroup, SELECT_SUMS_ROUND tile sums a
//                  round, a carry between rounds), select_scan_tiles (the tile's own scan on top of its base).  After it
//                  dst[r] is where record r goes and dst[n] the total; a dropped record has dst[r] == dst[r + 1].
//   select_gather  a lane owns 16 bytes of the OUTPUT: it finds the record those bytes belong to and builds them from
//                  aligned loads of the source.
//
// Offsets within a block fit 32 bits (a block is below 4 GiB: engine.hip's submit paths, FEED_SUB_MAX).
#pragma once

#include "tally_kernels.h"

namespace pssbam {

static constexpr uint32_t SELECT_SCAN_ITEMS = 4, SELECT_SCAN_THREADS = 256;
static constexpr uint32_t SELECT_SCAN_TILE = SELECT_SCAN_ITEMS * SELECT_SCAN_THREADS;   // entries of len[] per workgroup of the scan
static constexpr uint32_t SELECT_SUMS_ROUND = 256;                                      // tile sums per round of select_scan_sums
static constexpr uint32_t SELECT_GATHER_THREADS = 256, SELECT_GATHER_CHUNKS = 8;        // a workgroup's piece of the output: 256 x 8 x 16 B = 32 KiB

__device__ __forceinline__ uint32_t select_n_recs(const TallyParams &P) { return P.n_recs_dev ? min(*P.n_recs_dev, P.n_recs) : P.n_recs; }

// Was record r (below the block's count) added to the forward or the reverse main table?  The one statement of "kept" on the
// device: select_mark, coverage_add (coverage_kernels.h) and allele_add (allele_kernels.h) all ask it.  pl = the record's plan,
// rec_len = its bytes in the block, h = its decoded header.
__device__ __forceinline__ bool select_keep(const TallyParams &P, uint32_t r, GappedPlan &pl, uint32_t &rec_len, RecHdr &h) {
    const uint32_t o0 = P.offs[r], o1 = P.offs[r + 1];
    rec_len = o1 - o0;
    GlobalBytes src{P.recs + o0};
    h = decode_hdr(src, o1 - o0);
    if (P.gapped) pl = make_plan<true, false, true, true>(P, src, h);
    else static_cast<Plan &>(pl) = make_plan<true, true>(P, src, h);
    bool keep = (P.tally_mask & 1u) != 0 && (pl.pss_fwd || pl.pss_rev);
    if (keep && mism_on(P)) keep = !mism_beyond(P, count_mismatches(src, h, P.genome + pl.gbase, pl.s, pl.L, P.mism_tv != 0u));
    if (keep && P.score_w) keep = !score_below(P, read_score(P, src, h, P.genome + pl.gbase, pl.s, pl.L, pl.rev));
    return keep;
}
__device__ __forceinline__ bool select_keep(const TallyParams &P, uint32_t r, GappedPlan &pl, uint32_t &rec_len) {
    RecHdr h;
    return select_keep(P, r, pl, rec_len, h);
}

// len has P.n_recs + 1 entries (the host's bound of the count); the ones from the device's count on are zero
__global__ void __launch_bounds__(256) select_mark(const TallyParams P, uint32_t *len) {
    const uint32_t n = select_n_recs(P);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t r64 = blockIdx.x * blockDim.x + threadIdx.x; r64 <= P.n_recs; r64 += stride) {
        const uint32_t r = (uint32_t)r64;
        if (r >= n) { len[r] = 0u; continue; }
        GappedPlan pl;
        uint32_t rec_len;
        const bool keep = select_keep(P, r, pl, rec_len);
        len[r] = keep ? rec_len : 0u;
    }
}

// inclusive scan of a {bytes, records} pair over the workgroup; `lds` holds one pair per wave
__device__ __forceinline__ uint2 select_block_scan(uint2 v, uint2 *lds, uint2 &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t a = __shfl_up(v.x, d), b = __shfl_up(v.y, d);
        if (lane >= d) { v.x += a; v.y += b; }
    }
    __syncthreads();   // (lds may still be read from the call before)
    if (lane == 63u) lds[wave] = v;
    __syncthreads();
    uint2 base = make_uint2(0u, 0u);
    total = make_uint2(0u, 0u);
    for (uint32_t w = 0; w < n_waves; w++) {
        const uint2 s = lds[w];
        if (w < wave) { base.x += s.x; base.y += s.y; }
        total.x += s.x;
        total.y += s.y;
    }
    v.x += base.x;
    v.y += base.y;
    return v;
}

// sums[t] = {bytes, records} kept in tile t of len[0, n)
__global__ void __launch_bounds__(SELECT_SCAN_THREADS) select_tile_sums(const uint32_t *len, uint32_t n, uint2 *sums) {
    __shared__ uint2 lds[SELECT_SCAN_THREADS / 64];
    const uint32_t n_tiles = (n + SELECT_SCAN_TILE - 1) / SELECT_SCAN_TILE;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        uint2 v = make_uint2(0u, 0u);
        for (uint32_t k = 0; k < SELECT_SCAN_ITEMS; k++) {
            const uint32_t r = t * SELECT_SCAN_TILE + k * SELECT_SCAN_THREADS + threadIdx.x;
            const uint32_t l = r < n ? len[r] : 0u;
            v.x += l;
            v.y += l ? 1u : 0u;
        }
        uint2 total;
        (void)select_block_scan(v, lds, total);
        if (threadIdx.x == 0) sums[t] = total;
    }
}

// exclusive scan of the tile sums in place, one workgroup, a round of SELECT_SUMS_ROUND sums at a time; totals = {bytes, records}
__global__ void __launch_bounds__(SELECT_SUMS_ROUND) select_scan_sums(uint2 *sums, uint32_t n_tiles, unsigned long long *totals) {
    __shared__ uint2 lds[SELECT_SUMS_ROUND / 64];
    uint2 carry = make_uint2(0u, 0u);
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += SELECT_SUMS_ROUND) {
        const uint32_t t = t0 + threadIdx.x;
        const uint2 mine = t < n_tiles ? sums[t] : make_uint2(0u, 0u);
        uint2 total;
        const uint2 incl = select_block_scan(mine, lds, total);
        if (t < n_tiles) sums[t] = make_uint2(carry.x + incl.x - mine.x, carry.y + incl.y - mine.y);
        carry.x += total.x;
        carry.y += total.y;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry.x;
        totals[1] = carry.y;
    }
}

// len[0, n) becomes its exclusive scan, in place (a thread reads its entries before any is written, and tiles share
// none); dst[n] = the total.  A thread's entries are consecutive, so that the scan follows the input order.
__global__ void __launch_bounds__(SELECT_SCAN_THREADS) select_scan_tiles(uint32_t *len, uint32_t n, const uint2 *sums, const unsigned long long *totals) {
    __shared__ uint2 lds[SELECT_SCAN_THREADS / 64];
    const uint32_t n_tiles = (n + SELECT_SCAN_TILE - 1) / SELECT_SCAN_TILE;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint32_t r0 = t * SELECT_SCAN_TILE + threadIdx.x * SELECT_SCAN_ITEMS;
        uint32_t l[SELECT_SCAN_ITEMS];
        uint2 v = make_uint2(0u, 0u);
        for (uint32_t k = 0; k < SELECT_SCAN_ITEMS; k++) {
            l[k] = r0 + k < n ? len[r0 + k] : 0u;
            v.x += l[k];
        }
        uint2 total;
        const uint2 incl = select_block_scan(v, lds, total);
        uint32_t at = sums[t].x + incl.x - v.x;
        for (uint32_t k = 0; k < SELECT_SCAN_ITEMS; k++) {
            if (r0 + k < n) len[r0 + k] = at;
            at += l[k];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) len[n] = (uint32_t)totals[0];
}

// the record whose bytes hold output byte p: the last r of [lo, hi] with dst[r] <= p (dst[r + 1] > p then, since dst does
// not fall: the record is a kept one)
__device__ __forceinline__ uint32_t select_find(const uint32_t *dst, uint32_t lo, uint32_t hi, uint32_t p) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (dst[mid] <= p) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

// the dword at byte `at` of the source block: two aligned loads and a byte shift.  recs is 16-byte aligned; the second
// load is issued only when the dword does reach into it: an aligned word is read only when it holds a byte that was asked for
// (up to 3 bytes of it may lie behind the record or the block: same word as a valid byte, so the load cannot fault).
__device__ __forceinline__ uint32_t select_load_u32(const uint8_t *recs, uint32_t at) {
    const uint32_t *q = (const uint32_t *)(recs + (at & ~3u));
    const uint32_t sh = at & 3u;
    const uint32_t lo = q[0];
    return sh ? __builtin_amdgcn_alignbyte(q[1], lo, sh) : lo;
}

// Every lane owns 16 bytes of the output at a 16-byte aligned place (out is aligned; the total is rounded up, the bytes behind it are
// zero): a wave's store is one aligned KiB whatever the record boundaries are.  The workgroup narrows the record range
// of its 32 KiB piece once (two searches over all of dst, the same addresses in every lane); a lane then finds its own
// record in that range and reads the source at the record's own alignment.
__global__ void __launch_bounds__(SELECT_GATHER_THREADS) select_gather(const uint8_t *recs, const uint32_t *offs, const uint32_t *dst, uint32_t n,
                                                                        const unsigned long long *totals, uint8_t *out) {
    const uint32_t total = (uint32_t)totals[0];
    const uint32_t n_chunks = (uint32_t)(((uint64_t)total + 15ull) / 16ull);
    constexpr uint32_t PIECE = SELECT_GATHER_THREADS * SELECT_GATHER_CHUNKS;
    const uint32_t n_pieces = (n_chunks + PIECE - 1) / PIECE;
    for (uint32_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {
        const uint32_t c0 = piece * PIECE, c1 = min(c0 + PIECE, n_chunks);
        const uint32_t p_last = (uint32_t)min((uint64_t)c1 * 16ull, (uint64_t)total) - 1u;
        const uint32_t r_lo = select_find(dst, 0u, n - 1u, c0 * 16u), r_hi = select_find(dst, r_lo, n - 1u, p_last);
        for (uint32_t c = c0 + threadIdx.x; c < c1; c += SELECT_GATHER_THREADS) {
            const uint32_t p = c * 16u;   // (< total <= 2^32 - 16: no wrap)
            uint32_t r = select_find(dst, r_lo, r_hi, p);
            uint32_t d0 = dst[r], d1 = dst[r + 1u], o = offs[r];
            uint4 v;
            if ((uint64_t)p + 16ull <= d1) {   // the whole chunk is of one record: four dwords and one more for the shift
                const uint32_t at = o + (p - d0), sh = at & 3u;
                const Quad q = *(const Quad *)(recs + (at & ~3u));
                if (sh) {
                    const uint32_t q4 = *(const uint32_t *)(recs + (at & ~3u) + 16u);
                    v.x = __builtin_amdgcn_alignbyte(q.v[1], q.v[0], sh);
                    v.y = __builtin_amdgcn_alignbyte(q.v[2], q.v[1], sh);
                    v.z = __builtin_amdgcn_alignbyte(q.v[3], q.v[2], sh);
                    v.w = __builtin_amdgcn_alignbyte(q4, q.v[3], sh);
                } else {
                    v = make_uint4(q.v[0], q.v[1], q.v[2], q.v[3]);
                }
            } else {   // a record ends in the chunk: dword by dword, and the dword a boundary falls in byte by byte
                uint32_t w[4];
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t pk = p + 4u * k;
                    w[k] = 0u;
                    if (pk >= total) continue;
                    if (pk >= d1) {
                        r = select_find(dst, r, r_hi, pk);
                        d0 = dst[r]; d1 = dst[r + 1u]; o = offs[r];
                    }
                    if ((uint64_t)pk + 4ull <= d1) {
                        w[k] = select_load_u32(recs, o + (pk - d0));
                    } else {
                        for (uint32_t b = 0; b < 4u && pk + b < total; b++) {
                            if (pk + b >= d1) {
                                r = select_find(dst, r, r_hi, pk + b);
                                d0 = dst[r]; d1 = dst[r + 1u]; o = offs[r];
                            }
                            w[k] |= (uint32_t)recs[o + (pk + b - d0)] << (8u * b);
                        }
                    }
                }
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4 *)(out + (size_t)p) = v;
        }
    }
}

}  // namespace pssbam

// pss-bam_amd/csrc/coverage_kernels.h -- depth of coverage of the kept records (pssbam_engine_set_coverage, pss-bam -c / -b).
//
// One array uint32_t cov[stored genome length], indexed like P.genome, holds DIFFERENCES: a kept record (select_keep: exactly what
// the record sink delivers) with reference start s and length L on the contig at `lo` adds 1 at lo + s and 0xFFFFFFFF (-1 mod 2^32)
// at lo + s + L.  A kept record has s + L + 2 <= its contig's length (plan_head), so both entries lie inside the contig, every
// contig's differences sum to zero, and nothing is ever added in the padding between contigs: ONE inclusive prefix sum over the
// whole array, mod 2^32, is the depth inside every contig and 0 across every padding -- no segmented scan.  Depth is exact below
// 2^32 kept records over one position; beyond that it wraps.  The depth array itself is never stored.
//
//   coverage_add        lane per record, behind the block's tally kernels: the decision of select_mark, then two relaxed agent-scope
//                       atomic adds whose results are not used.  No lane waits on another.
//   finish (any number of times; nothing of the array changes):
//   coverage_tile_sums  sums[t] = the sum of the differences of tile t (COV_TILE positions, dwordx4 loads)
//   coverage_scan_sums  exclusive scan of per-tile values in place: one workgroup, COV_SUMS_ROUND values a round, a carry between
//                       rounds (the shape of select_scan_sums; no workgroup waits on another).  Used for the tile sums and, for the
//                       runs, for the per-tile run counts.
//   coverage_stats      every tile again on top of its base, depth in registers: the histogram 0..255 / above through LDS,
//                       per-contig {covered, depth_sum, max_depth} through LDS accumulators that live across the workgroup's
//                       tiles (one global atomic per workgroup and contig), and the tile's number of runs.
//   coverage_runs       (bedGraph only) {contig, start, depth} of every run and the end of the run before it, compacted, in order.
//   coverage_windows    (pss-bam -w only) every tile once more on top of its base, beside the genome's stored bytes: {depth_sum,
//                       covered, acgt, gc} of every fixed window of every listed contig, through LDS accumulators of the windows a
//                       tile meets and one no-return atomic per tile, window and non-zero word (at the end of the file).
//
// A run starts where the difference is non-zero and the depth is non-zero, and ends at the next non-zero difference: run boundaries
// are exactly the non-zero entries of cov[], so runs are maximal by construction and -- the depth being 0 in padding -- never cross a
// contig.  Positions in padding belong to no contig and count nowhere: a lane's contig comes from the list of the reference list's
// contigs sorted by `lo` ({lo low, lo high, length, unused}), which a workgroup narrows once per tile.
#pragma once

#include "select_kernels.h"

namespace pssbam {

static constexpr uint32_t COV_THREADS = 256, COV_ITEMS = 16;         // a lane owns 16 consecutive positions: four dwordx4 loads
static constexpr uint32_t COV_TILE = COV_THREADS * COV_ITEMS;        // positions per tile
static constexpr uint32_t COV_SUMS_ROUND = 256;                      // per-tile values per round of coverage_scan_sums
static constexpr uint32_t COV_HIST_BINS = 257;                       // depth 0..255, and above
static constexpr uint32_t COV_TILE_CONTIGS = 24;                     // LDS accumulators (a contig takes >= 512 stored positions: at most 9 meet a tile)
static constexpr uint32_t COV_OUT_RUNS = COV_HIST_BINS;              // out[]: the histogram, the number of runs, then 3 words per listed contig
static constexpr uint32_t COV_OUT_CONTIGS = COV_HIST_BINS + 1;

__device__ __forceinline__ void coverage_atomic_add(uint32_t *p, uint32_t v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (result unused: the no-return form)
}

// cov has cov_len entries, at least the stored genome's.  Both entries of a kept record are inside its contig (above), so the
// bound below never holds for a record the sink delivers: it is there only so that a wrong reference table cannot make the
// kernel write outside the array.
__global__ void __launch_bounds__(256) coverage_add(const TallyParams P, uint32_t *cov, uint64_t cov_len) {
    const uint32_t n = select_n_recs(P);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t r64 = blockIdx.x * blockDim.x + threadIdx.x; r64 < n; r64 += stride) {
        GappedPlan pl;
        uint32_t rec_len;
        if (!select_keep(P, (uint32_t)r64, pl, rec_len)) continue;
        const uint64_t a = pl.gbase + (uint64_t)(uint32_t)pl.s, b = a + pl.L;
        if (b >= cov_len) continue;
        coverage_atomic_add(cov + a, 1u);
        coverage_atomic_add(cov + b, 0xFFFFFFFFu);
    }
}

struct CovItems {
    uint32_t d[COV_ITEMS];
};

// the lane's 16 differences of tile t (cov is allocated in whole tiles and 16-byte aligned)
__device__ __forceinline__ CovItems coverage_load(const uint32_t *cov, uint64_t t) {
    const uint4 *q = (const uint4 *)(cov + t * COV_TILE + (uint64_t)threadIdx.x * COV_ITEMS);
    CovItems v;
    for (uint32_t k = 0; k < COV_ITEMS / 4; k++) {
        const uint4 w = q[k];
        v.d[4 * k] = w.x; v.d[4 * k + 1] = w.y; v.d[4 * k + 2] = w.z; v.d[4 * k + 3] = w.w;
    }
    return v;
}

// inclusive scan of one word over the workgroup (mod 2^32); `lds` holds one word per wave
__device__ __forceinline__ uint32_t coverage_block_scan(uint32_t v, uint32_t *lds, uint32_t &total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t a = __shfl_up(v, d);
        if (lane >= d) v += a;
    }
    __syncthreads();   // (lds may still be read from the call before)
    if (lane == 63u) lds[wave] = v;
    __syncthreads();
    uint32_t base = 0u;
    total = 0u;
    for (uint32_t w = 0; w < n_waves; w++) {
        const uint32_t s = lds[w];
        if (w < wave) base += s;
        total += s;
    }
    return v + base;
}

__global__ void __launch_bounds__(COV_THREADS) coverage_tile_sums(const uint32_t *cov, uint64_t n_tiles, unsigned long long *sums) {
    __shared__ uint32_t lds[COV_THREADS / 64];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const CovItems v = coverage_load(cov, t);
        uint32_t s = 0u;
        for (uint32_t k = 0; k < COV_ITEMS; k++) s += v.d[k];
        uint32_t total;
        (void)coverage_block_scan(s, lds, total);
        if (threadIdx.x == 0) sums[t] = total;
    }
}

// exclusive scan of vals[0, n) in place, one workgroup; *total (may be NULL) = the sum
__global__ void __launch_bounds__(COV_SUMS_ROUND) coverage_scan_sums(unsigned long long *vals, uint64_t n, unsigned long long *total) {
    __shared__ unsigned long long lds[COV_SUMS_ROUND / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long carry = 0ull;
    for (uint64_t t0 = 0; t0 < n; t0 += COV_SUMS_ROUND) {
        const uint64_t t = t0 + threadIdx.x;
        const unsigned long long mine = t < n ? vals[t] : 0ull;
        unsigned long long v = mine;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const unsigned long long a = __shfl_up(v, d);
            if (lane >= d) v += a;
        }
        __syncthreads();
        if (lane == 63u) lds[wave] = v;
        __syncthreads();
        unsigned long long base = 0ull, round = 0ull;
        for (uint32_t w = 0; w < COV_SUMS_ROUND / 64; w++) {
            const unsigned long long s = lds[w];
            if (w < wave) base += s;
            round += s;
        }
        if (t < n) vals[t] = carry + base + v - mine;
        carry += round;
    }
    if (total && threadIdx.x == 0) *total = carry;
}

__device__ __forceinline__ uint64_t coverage_contig_lo(const uint4 c) { return ((uint64_t)c.y << 32) | c.x; }

// the first contig of [lo, hi) that ends behind position p (hi when none does)
__device__ __forceinline__ uint32_t coverage_find(const uint4 *contigs, uint32_t lo, uint32_t hi, uint64_t p) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const uint4 c = contigs[mid];
        if (coverage_contig_lo(c) + c.z > p) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// the lane's depths of tile t: d[] becomes the depth at each of its positions; returns the depth in front of the first
__device__ __forceinline__ uint32_t coverage_depths(CovItems &v, const CovItems &diff, uint32_t tile_base, uint32_t *lds) {
    uint32_t s = 0u;
    for (uint32_t k = 0; k < COV_ITEMS; k++) s += diff.d[k];
    uint32_t total;
    const uint32_t incl = coverage_block_scan(s, lds, total);
    const uint32_t before = tile_base + incl - s;
    uint32_t at = before;
    for (uint32_t k = 0; k < COV_ITEMS; k++) {
        at += diff.d[k];
        v.d[k] = at;
    }
    return before;
}

// out: COV_HIST_BINS histogram words, the number of runs, then {covered, depth_sum, max_depth} per listed contig; run_cnt[t] = the
// runs that start in tile t
__global__ void __launch_bounds__(COV_THREADS) coverage_stats(const uint32_t *cov, uint64_t n_tiles, const unsigned long long *base, const uint4 *contigs,
                                                              uint32_t n_contigs, unsigned long long *out, unsigned long long *run_cnt) {
    __shared__ uint32_t lds[COV_THREADS / 64];
    __shared__ uint32_t hist[COV_HIST_BINS];
    __shared__ unsigned long long c_sum[COV_TILE_CONTIGS], c_cov[COV_TILE_CONTIGS], zeros_lds;
    __shared__ uint32_t c_max[COV_TILE_CONTIGS];
    for (uint32_t i = threadIdx.x; i < COV_HIST_BINS; i += COV_THREADS) hist[i] = 0u;
    if (threadIdx.x < COV_TILE_CONTIGS) { c_sum[threadIdx.x] = 0ull; c_cov[threadIdx.x] = 0ull; c_max[threadIdx.x] = 0u; }
    // The LDS accumulators stand for the contigs acc_lo .. acc_lo + COV_TILE_CONTIGS - 1 and live across the workgroup's tiles: they
    // go to the totals -- one atomic per workgroup and contig -- only when a tile brings a contig outside that window (a workgroup's
    // tiles lie a whole grid apart, so on a genome of few long contigs that is a handful of times), and at the end.
    uint32_t acc_lo = 0xFFFFFFFFu;   // (the same in every lane)
    auto to_totals = [&]() {
        if (threadIdx.x < COV_TILE_CONTIGS && c_cov[threadIdx.x]) {
            unsigned long long *o = out + COV_OUT_CONTIGS + 3ull * (acc_lo + threadIdx.x);
            atomicAdd(o, c_cov[threadIdx.x]);
            atomicAdd(o + 1, c_sum[threadIdx.x]);
            atomicMax(o + 2, (unsigned long long)c_max[threadIdx.x]);
            c_sum[threadIdx.x] = 0ull; c_cov[threadIdx.x] = 0ull; c_max[threadIdx.x] = 0u;
        }
    };
    uint64_t zeros = 0, wg_runs = 0;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const CovItems diff = coverage_load(cov, t);
        const uint64_t p_tile = t * COV_TILE, p0 = p_tile + (uint64_t)threadIdx.x * COV_ITEMS;
        const uint32_t c_lo = coverage_find(contigs, 0u, n_contigs, p_tile);               // the same addresses in every lane
        const uint32_t c_hi = coverage_find(contigs, c_lo, n_contigs, p_tile + COV_TILE - 1u);   // the last contig that may meet the tile (or n_contigs)
        if (acc_lo == 0xFFFFFFFFu || c_lo < acc_lo || c_hi >= acc_lo + COV_TILE_CONTIGS) {   // (the lanes' adds of the tile before are behind its last barrier)
            to_totals();
            acc_lo = c_lo;
        }
        CovItems dep;
        const uint32_t before = coverage_depths(dep, diff, (uint32_t)base[t], lds);   // (its barriers also order the zeroing above)
        uint32_t idx = coverage_find(contigs, c_lo, min(c_hi + 1u, n_contigs), p0);
        uint4 c = idx < n_contigs ? contigs[idx] : make_uint4(0u, 0u, 0u, 0u);
        uint32_t n_cov = 0u, d_max = 0u, runs = 0u;
        uint64_t d_sum = 0;
        auto flush = [&]() {
            if (!n_cov) return;
            const uint32_t slot = idx - acc_lo;
            if (slot < COV_TILE_CONTIGS) {
                atomicAdd(&c_cov[slot], (unsigned long long)n_cov);
                atomicAdd(&c_sum[slot], (unsigned long long)d_sum);
                atomicMax(&c_max[slot], d_max);
            } else {   // (more contigs in a tile than the stored layout allows: straight to the totals)
                unsigned long long *o = out + COV_OUT_CONTIGS + 3ull * idx;
                atomicAdd(o, (unsigned long long)n_cov);
                atomicAdd(o + 1, (unsigned long long)d_sum);
                atomicMax(o + 2, (unsigned long long)d_max);
            }
            n_cov = 0u; d_max = 0u; d_sum = 0;
        };
        // the common lane: all of its positions inside one contig and no difference among them -- one depth, sixteen times
        uint32_t any = 0u;
        for (uint32_t k = 0; k < COV_ITEMS; k++) any |= diff.d[k];
        const bool plain = !any && idx < n_contigs && p0 >= coverage_contig_lo(c) && p0 + COV_ITEMS <= coverage_contig_lo(c) + c.z;
        if (plain) {
            if (!before) zeros += COV_ITEMS;
            else {
                atomicAdd(&hist[min(before, COV_HIST_BINS - 1u)], COV_ITEMS);
                n_cov = COV_ITEMS;
                d_sum = (uint64_t)before * COV_ITEMS;
                d_max = before;
            }
        }
        for (uint32_t k = 0; k < COV_ITEMS && !plain; k++) {
            const uint64_t p = p0 + k;
            while (idx < n_contigs && p >= coverage_contig_lo(c) + c.z) {
                flush();
                idx++;
                if (idx < n_contigs) c = contigs[idx];
            }
            const uint32_t d = dep.d[k];
            if (diff.d[k] && d) runs++;
            if (idx >= n_contigs || p < coverage_contig_lo(c)) continue;   // padding
            if (!d) { zeros++; continue; }
            atomicAdd(&hist[min(d, COV_HIST_BINS - 1u)], 1u);
            n_cov++;
            d_sum += d;
            d_max = max(d_max, d);
        }
        flush();
        uint32_t tile_runs;
        (void)coverage_block_scan(runs, lds, tile_runs);   // (its barriers also close the LDS accumulators)
        if (threadIdx.x == 0) { run_cnt[t] = tile_runs; wg_runs += tile_runs; }
    }
    to_totals();
    // depth 0 is counted in a register: one LDS add per lane, not one per position
    if (threadIdx.x == 0) zeros_lds = 0ull;
    __syncthreads();
    if (zeros) atomicAdd(&zeros_lds, (unsigned long long)zeros);
    __syncthreads();
    if (threadIdx.x == 0 && zeros_lds) atomicAdd(out, zeros_lds);
    for (uint32_t i = threadIdx.x; i < COV_HIST_BINS; i += COV_THREADS)
        if (hist[i]) atomicAdd(out + i, (unsigned long long)hist[i]);
    if (threadIdx.x == 0 && wg_runs) atomicAdd(out + COV_OUT_RUNS, (unsigned long long)wg_runs);
}

// run i (in genome order) = {slot[i]: its contig's place in the list, start[i]: contig-relative, depth[i]}; end[i] is written by
// whoever holds the next non-zero difference, possibly in a later tile: no lane waits for it.  run_base = the scanned run counts.
__global__ void __launch_bounds__(COV_THREADS) coverage_runs(const uint32_t *cov, uint64_t n_tiles, const unsigned long long *base, const unsigned long long *run_base,
                                                             const uint4 *contigs, uint32_t n_contigs, uint64_t n_runs, uint32_t *slot, uint32_t *start,
                                                             uint32_t *end, uint32_t *depth) {
    __shared__ uint32_t lds[COV_THREADS / 64];
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const CovItems diff = coverage_load(cov, t);
        CovItems dep;
        (void)coverage_depths(dep, diff, (uint32_t)base[t], lds);
        uint32_t runs = 0u;
        for (uint32_t k = 0; k < COV_ITEMS; k++) runs += diff.d[k] && dep.d[k] ? 1u : 0u;
        uint32_t tile_runs;
        const uint32_t incl = coverage_block_scan(runs, lds, tile_runs);
        uint64_t at = run_base[t] + (incl - runs);   // runs that start in front of this lane's positions
        const uint64_t p0 = t * COV_TILE + (uint64_t)threadIdx.x * COV_ITEMS;
        uint32_t idx = 0xFFFFFFFFu;
        uint4 c = make_uint4(0u, 0u, 0u, 0u);
        for (uint32_t k = 0; k < COV_ITEMS; k++) {
            if (!diff.d[k]) continue;
            const uint64_t p = p0 + k;
            if (idx == 0xFFFFFFFFu || p >= coverage_contig_lo(c) + c.z) {   // (few entries are non-zero: a search each time one leaves the contig at hand)
                idx = coverage_find(contigs, 0u, n_contigs, p);
                c = idx < n_contigs ? contigs[idx] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
            }
            const uint32_t rel = (uint32_t)(p - coverage_contig_lo(c));   // (the closing entry of a run lies in the run's contig)
            if (dep.d[k] - diff.d[k] != 0u && at >= 1u && at - 1u < n_runs) end[at - 1u] = rel;   // the depth in front was non-zero: a run ends here
            if (dep.d[k] && at < n_runs) {
                slot[at] = idx < n_contigs && p >= coverage_contig_lo(c) ? idx : 0xFFFFFFFFu;
                start[at] = rel;
                depth[at] = dep.d[k];
                at++;
            }
        }
    }
}

// ---- fixed windows (pssbam_engine_finish_coverage_windows, pss-bam -w) ----------------------------------------------------------------
// Every listed contig is cut into windows [k W, min((k + 1) W, length)); the window k of the contig at place c of the list has the
// global id wbase[c] + k (wbase: the host's prefix of ceil(length / W)), so ids rise with the position and the windows a tile meets
// are one stretch of ids behind w_first.  The accumulators are four arrays over the ids -- an atomic wave-instruction then adds to
// consecutive words -- in `shards` copies of n entries each: workgroup b adds to copy b % shards and the host sums the copies.  With
// few, large windows every workgroup at work adds to the same handful of words, and adds to one address take their turns.
struct CovWindows {
    unsigned long long *depth_sum;
    uint32_t *covered, *acgt, *gc;
    uint64_t n;                       // ids at and above n are never written
    uint32_t shards;
};

// A stretch of n positions of one contig meets at most (n + 14) / 16 + 1 windows of 16 or more, and at most 9 contigs meet a tile.
static constexpr uint32_t COV_TILE_WINDOWS = (COV_TILE + 9 * 14) / 16 + 1 + 9;

__device__ __forceinline__ void coverage_atomic_add64(unsigned long long *p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// of the four stored genome bytes in x: how many are A C G T (below 4), and how many of those C or G (1 or 2)
__device__ __forceinline__ void coverage_count_bases(uint32_t x, uint32_t &n_acgt, uint32_t &n_gc) {
    const uint32_t t = x & 0xFCFCFCFCu;
    const uint32_t other = ((((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) >> 7) & 0x01010101u;   // 1 per byte of 4 and above (no carry leaves a byte)
    n_acgt += 4u - __popc(other);
    n_gc += __popc((x ^ (x >> 1)) & 0x01010101u & ~other);
}

// Walks the tiles like coverage_stats and adds {depth_sum, covered, acgt, gc} of every window of W positions to out.  A lane sums
// in registers while contig and window stay the same; what it has goes to the workgroup's LDS accumulators of the tile's windows, and
// those -- what is non-zero of them -- to the totals once per tile and window.  genome has genome_len stored bytes, a multiple of 16.
__global__ void __launch_bounds__(COV_THREADS) coverage_windows(const uint32_t *cov, const uint8_t *genome, uint64_t genome_len, uint64_t n_tiles,
                                                                const unsigned long long *base, const uint4 *contigs, uint32_t n_contigs,
                                                                const unsigned long long *wbase, uint32_t W, CovWindows out) {
    __shared__ uint32_t lds[COV_THREADS / 64];
    __shared__ unsigned long long w_sum[COV_TILE_WINDOWS];
    __shared__ uint32_t w_cov[COV_TILE_WINDOWS], w_acgt[COV_TILE_WINDOWS], w_gc[COV_TILE_WINDOWS];
    for (uint32_t i = threadIdx.x; i < COV_TILE_WINDOWS; i += COV_THREADS) { w_sum[i] = 0ull; w_cov[i] = 0u; w_acgt[i] = 0u; w_gc[i] = 0u; }
    const uint64_t copy = (uint64_t)(blockIdx.x % out.shards) * out.n;   // the workgroup's copy of the accumulators
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const CovItems diff = coverage_load(cov, t);
        const uint64_t p_tile = t * COV_TILE, p0 = p_tile + (uint64_t)threadIdx.x * COV_ITEMS;
        const uint4 g = p0 < genome_len ? *(const uint4 *)(genome + p0) : make_uint4(~0u, ~0u, ~0u, ~0u);   // (behind the genome lies no contig)
        const uint32_t gw[4] = {g.x, g.y, g.z, g.w};
        const uint32_t c_lo = coverage_find(contigs, 0u, n_contigs, p_tile);               // the same addresses in every lane
        const uint32_t c_hi = coverage_find(contigs, c_lo, n_contigs, p_tile + COV_TILE - 1u);
        uint64_t w_first = 0;                                                              // the id of the tile's first window
        if (c_lo < n_contigs) {
            const uint64_t lo0 = coverage_contig_lo(contigs[c_lo]);
            w_first = wbase[c_lo] + (p_tile > lo0 ? (uint32_t)(p_tile - lo0) / W : 0u);
        }
        CovItems dep;
        const uint32_t before = coverage_depths(dep, diff, (uint32_t)base[t], lds);   // (its barriers also order the zeroing above and below)
        uint32_t idx = coverage_find(contigs, c_lo, min(c_hi + 1u, n_contigs), p0);
        uint4 c = idx < n_contigs ? contigs[idx] : make_uint4(0u, 0u, 0u, 0u);
        // the window at hand: id wid, ends in front of genome position w_end (0: none)
        uint64_t wid = 0, w_end = 0, d_sum = 0;
        uint32_t n_cov = 0u, n_acgt = 0u, n_gc = 0u;
        auto flush = [&]() {
            if (n_cov | n_acgt) {
                const uint64_t slot = wid - w_first;
                if (slot < COV_TILE_WINDOWS) {
                    if (d_sum) atomicAdd(&w_sum[slot], (unsigned long long)d_sum);
                    if (n_cov) atomicAdd(&w_cov[slot], n_cov);
                    if (n_acgt) atomicAdd(&w_acgt[slot], n_acgt);
                    if (n_gc) atomicAdd(&w_gc[slot], n_gc);
                } else if (wid < out.n) {   // (more windows in a tile than the stored layout allows: straight to the totals)
                    if (d_sum) coverage_atomic_add64(out.depth_sum + copy + wid, d_sum);
                    if (n_cov) coverage_atomic_add(out.covered + copy + wid, n_cov);
                    if (n_acgt) coverage_atomic_add(out.acgt + copy + wid, n_acgt);
                    if (n_gc) coverage_atomic_add(out.gc + copy + wid, n_gc);
                }
            }
            n_cov = 0u; n_acgt = 0u; n_gc = 0u; d_sum = 0;
        };
        auto enter = [&](uint64_t p) {   // p lies in contig idx and behind the window at hand
            flush();
            const uint64_t lo = coverage_contig_lo(c);
            const uint32_t k = (uint32_t)(p - lo) / W;
            wid = wbase[idx] + k;
            w_end = lo + min((uint64_t)(k + 1u) * W, (uint64_t)c.z);
        };
        // the common lane: all of its positions inside one window and no difference among them -- one depth, sixteen times, and the
        // bases counted a word at a time
        uint32_t any = 0u;
        for (uint32_t k = 0; k < COV_ITEMS; k++) any |= diff.d[k];
        bool plain = !any && idx < n_contigs && p0 >= coverage_contig_lo(c) && p0 + COV_ITEMS <= coverage_contig_lo(c) + c.z;
        if (plain) {
            enter(p0);
            plain = p0 + COV_ITEMS <= w_end;
        }
        if (plain) {
            for (uint32_t k = 0; k < 4u; k++) coverage_count_bases(gw[k], n_acgt, n_gc);
            if (before) { n_cov = COV_ITEMS; d_sum = (uint64_t)before * COV_ITEMS; }
        }
#pragma unroll
        for (uint32_t k = 0; k < COV_ITEMS; k++) {
            if (plain) break;
            const uint64_t p = p0 + k;
            while (idx < n_contigs && p >= coverage_contig_lo(c) + c.z) {
                flush();
                w_end = 0;
                idx++;
                if (idx < n_contigs) c = contigs[idx];
            }
            if (idx >= n_contigs || p < coverage_contig_lo(c)) continue;   // padding
            if (p >= w_end) enter(p);
            const uint32_t b = (gw[k >> 2] >> (8u * (k & 3u))) & 0xFFu, d = dep.d[k];
            n_acgt += b < 4u ? 1u : 0u;
            n_gc += b == 1u || b == 2u ? 1u : 0u;
            n_cov += d ? 1u : 0u;
            d_sum += d;
        }
        // what the lane holds at its end: when the whole wave holds the same window -- every wave of a tile inside a large window
        // -- the wave sums first and one lane adds
        const uint64_t wid0 = __shfl(wid, 0);
        if (__all(w_end != 0 && wid == wid0)) {
            uint32_t bases = n_acgt | (n_gc << 16);   // (at most 1024 each)
            for (uint32_t m = 1; m < 64u; m <<= 1) {
                d_sum += __shfl_xor(d_sum, m);
                n_cov += __shfl_xor(n_cov, m);
                bases += __shfl_xor(bases, m);
            }
            if (threadIdx.x & 63u) { d_sum = 0; n_cov = 0u; bases = 0u; }
            n_acgt = bases & 0xFFFFu;
            n_gc = bases >> 16;
        }
        flush();
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < COV_TILE_WINDOWS; i += COV_THREADS) {
            const uint64_t w = w_first + i;
            if (!(w_cov[i] | w_acgt[i])) continue;
            if (w < out.n) {
                if (w_sum[i]) coverage_atomic_add64(out.depth_sum + copy + w, w_sum[i]);
                if (w_cov[i]) coverage_atomic_add(out.covered + copy + w, w_cov[i]);
                if (w_acgt[i]) coverage_atomic_add(out.acgt + copy + w, w_acgt[i]);
                if (w_gc[i]) coverage_atomic_add(out.gc + copy + w, w_gc[i]);
            }
            w_sum[i] = 0ull; w_cov[i] = 0u; w_acgt[i] = 0u; w_gc[i] = 0u;
        }
    }
}

}  // namespace pssbam

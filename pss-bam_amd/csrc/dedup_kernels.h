// pss-bam_amd/csrc/dedup_kernels.h -- duplicate flagging (pssbam_engine_set_duplicates, pss-bam -d, fragkon -d): the engine sets FLAG
// bit 0x400 of the duplicates in its device copy of a block, in front of the block's tally kernels, so that every tally and select
// kernel sees the deduplicated input and none of them is touched.
//
// The definition (include/pssbam_hip.h):
//   input order   the order of the submit calls, and the record order inside each block.
//   eligible      an unpaired record (FLAG 0x1 clear) that is a candidate of the run's own tool: on a PSSBAM_TALLY_PSS engine pss_cand
//                 as the plain make_plan leaves it, on a PSSBAM_TALLY_KMER engine fk5 || fk3 -- not dropped by the read-group
//                 filter, not a parse skip, contig known, none of 0x4 0x100 0x200 0x400 0x800, CIGAR exactly <L>M, mapping quality,
//                 the length window, the contig-edge test and the -T regions when set.  The content filters (-y, -n / -V, -Q, and the
//                 -U / -D context test) take no part: they apply after deduplication.
//   key           (refID, POS, L, FLAG & 0x10, g): L the SEQ length, g the record's plane under read groups (0 = unassigned, 1 + index
//                 otherwise), else 0.
//   duplicate     an eligible record with an earlier eligible record of the same key, in input order, across all blocks since create
//                 or reset.  The first record of a key wins.  Paired, ineligible and already flagged records are never flagged
//                 here and shadow nothing.
//
// The table: open addressing, linear probing, a slot = {a, b, ord, count}, 32 bytes.  a = refID << 32 | POS and
// b = L | strand << 32 | g << 33 are the exact key (an eligible record has POS >= 0 and g < 2^13: neither word is ever all ones, the
// EMPTY mark); ord is the smallest ordinal (block sequence number << 32 | record index) among the key's records, count their number.
// The protocol never waits for another lane's store:
//   1. probe linearly from hash(a, b);
//   2. CAS a from EMPTY; on any old value but EMPTY and a itself, next slot;
//   3. CAS b from EMPTY; on any old value but EMPTY and b itself, next slot (the slot went to a rival with the same a);
//   4. the slot is the key's: atomicMin(ord), atomicAdd(count).
// A lane that claimed a goes on to CAS b in the same kernel, and only lanes with the same a do: a slot is never half written at
// a kernel boundary, and once both words stand they never change, so every record of a key ends in the same slot.  The probe loop is
// bounded by the capacity; running out sets DEDUP_FULL in the state word and the next engine call fails -- it never spins.  (The
// engine keeps the table at most half full.)
#pragma once

#include "tally_kernels.h"

namespace pssbam {

struct DedupSlot { unsigned long long a, b, ord, count; };
static_assert(sizeof(DedupSlot) == 32, "a slot is one 32-byte sector");
constexpr unsigned long long DEDUP_EMPTY = ~0ull;
constexpr unsigned long long DEDUP_FULL = 1ull << 63;     // state word: a probe loop ran out (bits 0..62: occupied slots)
constexpr uint32_t DEDUP_NO_SLOT = 0xFFFFFFFFu;           // slot_of[r] of an ineligible record
constexpr uint32_t DEDUP_CENSUS_LDS_BINS = 256;           // group sizes counted in LDS by dedup_census

__device__ __forceinline__ uint64_t dedup_hash(unsigned long long a, unsigned long long b) {   // (splitmix64's finalizer over both words)
    uint64_t x = a * 0x9E3779B97F4A7C15ull ^ (b + 0xD6E8FEB86659FD93ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// -> the key's slot, or DEDUP_NO_SLOT when the table is full; claimed: this lane wrote the slot's b (one lane per slot does)
__device__ __forceinline__ uint32_t dedup_find_slot(DedupSlot *table, uint32_t mask, unsigned long long a, unsigned long long b, bool &claimed) {
    uint32_t s = (uint32_t)dedup_hash(a, b) & mask;
    for (uint64_t k = 0; k <= mask; k++, s = (s + 1u) & mask) {
        const unsigned long long a0 = atomicCAS(&table[s].a, DEDUP_EMPTY, a);
        if (a0 != DEDUP_EMPTY && a0 != a) continue;
        const unsigned long long b0 = atomicCAS(&table[s].b, DEDUP_EMPTY, b);
        if (b0 != DEDUP_EMPTY && b0 != b) continue;
        claimed = b0 == DEDUP_EMPTY;
        return s;
    }
    return DEDUP_NO_SLOT;
}

// one add per wave of the lanes' flags (every lane of the wave calls it)
__device__ __forceinline__ void dedup_wave_count(unsigned long long *word, bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m && (threadIdx.x & 63u) == 0u) atomicAdd(word, (unsigned long long)__popcll(m));
}

// the table's slots [0, n) become empty
__global__ void __launch_bounds__(256) dedup_clear(DedupSlot *table, uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n; s += stride) {
        uint4 *q = (uint4 *)(table + s);
        q[0] = make_uint4(~0u, ~0u, ~0u, ~0u);   // a, b
        q[1] = make_uint4(~0u, ~0u, 0u, 0u);     // ord, count
    }
}

// Lane per record: slot_of[r] = the slot of record r's key, DEDUP_NO_SLOT when it is not eligible.  slot_of has P.n_recs entries (the
// host's bound of the count); the ones from the device's count on are DEDUP_NO_SLOT.  state: + the slots newly occupied.
__global__ void __launch_bounds__(256) dedup_insert(const TallyParams P, const PlaneParams G, uint32_t use_groups, DedupSlot *table, uint32_t mask,
                                                    uint32_t seq, uint32_t *slot_of, unsigned long long *state) {
    const uint32_t n = P.n_recs_dev ? min(*P.n_recs_dev, P.n_recs) : P.n_recs;
    const bool do_pss = (P.tally_mask & 1u) != 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = ((uint64_t)P.n_recs + stride - 1) / stride;   // the same for every lane: the wave stays whole for the ballots
    for (uint64_t i = 0; i < rounds; i++) {
        const uint64_t r64 = i * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const uint32_t r = (uint32_t)r64;
        bool claimed = false, full = false;
        if (r64 < P.n_recs) {
            uint32_t slot = DEDUP_NO_SLOT;
            if (r < n) {
                const uint32_t o0 = P.offs[r], o1 = P.offs[r + 1];
                GlobalBytes src{P.recs + o0};
                const RecHdr h = decode_hdr(src, o1 - o0);
                bool eligible;
                uint32_t L;
                if (do_pss) {
                    const Plan pl = make_plan<true, false>(P, src, h);
                    eligible = pl.pss_cand;
                    L = pl.L;
                } else {
                    const Plan pl = make_plan<false, true>(P, src, h);
                    eligible = pl.fk5 || pl.fk3;
                    L = pl.Lk;
                }
                eligible = eligible && !(h.flag & FL_PAIRED);
                if (eligible) {
                    const uint32_t g = use_groups ? read_group_plane(src, h, G) : 0u;
                    const unsigned long long a = (unsigned long long)(uint32_t)h.ref_id << 32 | (uint32_t)h.pos;
                    const unsigned long long b = (unsigned long long)L | (unsigned long long)((h.flag >> 4) & 1u) << 32 | (unsigned long long)g << 33;
                    slot = dedup_find_slot(table, mask, a, b, claimed);
                    if (slot != DEDUP_NO_SLOT) {
                        atomicMin(&table[slot].ord, (unsigned long long)seq << 32 | r);
                        atomicAdd(&table[slot].count, 1ull);
                    } else {
                        full = true;
                    }
                }
            }
            slot_of[r] = slot;
        }
        dedup_wave_count(state, claimed);
        if (__ballot(full) && (threadIdx.x & 63u) == 0u) atomicOr(state, DEDUP_FULL);
    }
}

// Lane per record, no second decode: an eligible record whose slot names another record as the key's first is a duplicate and gets
// FLAG bit 0x400 -- bit 0x04 of byte 19, the high byte of FLAG, a one-byte read-modify-write by the one lane that owns the record.
__global__ void __launch_bounds__(256) dedup_resolve(uint8_t *recs, const uint32_t *offs, uint32_t n_recs, const DedupSlot *table, uint32_t seq,
                                                     const uint32_t *slot_of) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r64 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r64 < n_recs; r64 += stride) {
        const uint32_t r = (uint32_t)r64, slot = slot_of[r];
        if (slot == DEDUP_NO_SLOT) continue;
        if (table[slot].ord != ((unsigned long long)seq << 32 | r)) {
            uint8_t *flag_hi = recs + offs[r] + 19u;   // (an eligible record is well formed: at least 36 bytes)
            *flag_hi = (uint8_t)(*flag_hi | 0x04u);
        }
    }
}

// Lane per slot of the old table: its key goes into the new one by the same protocol, with its ordinal and its count
__global__ void __launch_bounds__(256) dedup_rehash(const DedupSlot *old_table, uint64_t n_old, DedupSlot *table, uint32_t mask, unsigned long long *state) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n_old + stride - 1) / stride;
    for (uint64_t i = 0; i < rounds; i++) {
        const uint64_t s = i * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool full = false;
        if (s < n_old) {
            const DedupSlot o = old_table[s];
            if (o.a != DEDUP_EMPTY) {
                bool claimed;
                const uint32_t slot = dedup_find_slot(table, mask, o.a, o.b, claimed);
                if (slot != DEDUP_NO_SLOT) {
                    atomicMin(&table[slot].ord, o.ord);
                    atomicAdd(&table[slot].count, o.count);
                } else {
                    full = true;
                }
            }
        }
        if (__ballot(full) && (threadIdx.x & 63u) == 0u) atomicOr(state, DEDUP_FULL);
    }
}

// Lane per slot: out = {eligible records, distinct keys, hist[0 .. hist_max + 1]}; hist[c] = the keys with exactly c eligible records,
// hist[hist_max + 1] the keys with more.  Sizes below DEDUP_CENSUS_LDS_BINS are counted per workgroup first.
__global__ void __launch_bounds__(256) dedup_census(const DedupSlot *table, uint64_t n, uint32_t hist_max, unsigned long long *out) {
    __shared__ uint32_t lds[DEDUP_CENSUS_LDS_BINS];
    for (uint32_t i = threadIdx.x; i < DEDUP_CENSUS_LDS_BINS; i += blockDim.x) lds[i] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t rounds = (n + stride - 1) / stride;
    unsigned long long records = 0ull;
    uint32_t keys = 0u;
    for (uint64_t i = 0; i < rounds; i++) {
        const uint64_t s = i * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (s >= n) continue;
        const DedupSlot o = table[s];
        if (o.a == DEDUP_EMPTY) continue;
        records += o.count;
        keys++;
        const uint32_t bin = (uint32_t)min(o.count, (unsigned long long)hist_max + 1ull);
        if (bin < DEDUP_CENSUS_LDS_BINS) atomicAdd(&lds[bin], 1u);
        else atomicAdd(&out[2u + bin], 1ull);
    }
    if (records) atomicAdd(&out[0], records);
    if (keys) atomicAdd(&out[1], (unsigned long long)keys);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < DEDUP_CENSUS_LDS_BINS && i <= hist_max + 1u; i += blockDim.x)
        if (lds[i]) atomicAdd(&out[2u + i], (unsigned long long)lds[i]);
}

}  // namespace pssbam

// pss-bam_amd/csrc/end_mask_kernels.h -- the end mask of the record and the block sink (pssbam_engine_set_end_mask, pss-bam -K):
// behind select_gather and in front of the deflate, the first n5 bases of the 5' end and the first n3 bases of the 3' end of every
// kept record become N with quality 0 in the output copy -- all of them (PSSBAM_END_MASK_ALL), or only those that look like
// deamination: T at the 5' and A at the 3' end of the read as it was sequenced (DS), T at both (SS).  DESIGN 4.2u.
//
//   pssbam_end_mask_record   one record: header fields, bounds rule, the two regions.  Plain C that also compiles as HIP device
//                            code, so that host/hostcheck_main.c and tools/end_mask_emulate.cpp run the kernel's own logic.
//   select_mask_ends         a lane per input record of the block, dst[] of the scan tells it where its copy starts.
//
// Writes are single bytes.  A lane reads a SEQ byte, sets one or both nibbles and stores that byte; it stores single QUAL bytes.
// Every byte it stores lies in [rec + seq_at, rec + qual_at + l_seq) of its own record, records do not overlap in the output,
// and a record has one lane: no byte has two writers.  Nothing wider is stored, because a wider read-modify-write is not owned:
// a record's last QUAL byte can share a dword with the next record's block_size (no aux fields), and the 16 bytes a lane of
// select_gather owns hold several short records.  Byte stores cost nothing here that matters: a record has at most
// min(n5, l) + min(n3, l) masked positions, a handful, against the hundreds of bytes select_gather moved for it.
#ifndef PSSBAM_END_MASK_KERNELS_H
#define PSSBAM_END_MASK_KERNELS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PSSBAM_EM_FN __host__ __device__ __forceinline__
#else
#define PSSBAM_EM_FN static inline
#endif

#define PSSBAM_EM_OFF 0
#define PSSBAM_EM_ALL 1
#define PSSBAM_EM_DS 2
#define PSSBAM_EM_SS 3
#define PSSBAM_EM_MAX_N 65535u

/* a little-endian dword at any alignment (records start anywhere in the output) */
PSSBAM_EM_FN uint32_t pssbam_em_u32(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

/* positions [a, b) of SEQ: the ones whose code is `code` (0: every one) become N, their quality 0 (qual == NULL: left alone) */
PSSBAM_EM_FN void pssbam_em_range(uint8_t *seq, uint8_t *qual, uint32_t a, uint32_t b, uint32_t code)
{
    if (a >= b) return;
    for (uint32_t k = a >> 1; k <= (b - 1u) >> 1; k++) {
        const uint32_t by = seq[k], i0 = 2u * k, i1 = i0 + 1u;
        uint32_t nb = by;
        if (i0 >= a && (!code || (by >> 4) == code)) {   /* (i0 < b: k is at most (b - 1) / 2) */
            nb |= 0xF0u;
            if (qual) qual[i0] = 0;
        }
        if (i1 < b && (!code || (by & 15u) == code)) {   /* (i1 > a; the pad nibble of an odd l_seq is position l_seq >= b) */
            nb |= 0x0Fu;
            if (qual) qual[i1] = 0;
        }
        if (nb != by) seq[k] = (uint8_t)nb;
    }
}

/* One record of `len` bytes at rec (block_size first), in place.  As stored, the head region [0, kh) is the 5' end of a forward
 * and the 3' end of a reverse read, the tail region [l - kt, l) the other one; in the read's own orientation DS asks for T at
 * the 5' and A at the 3' end, which on a reverse read are stored complemented and swapped: T in the head and A in the tail on
 * either strand.  SS asks for T at both ends: stored T on a forward, stored A on a reverse read.  The regions are walked one
 * after the other; a position of both is masked when either walk masks it (N meets no rule of the second walk, and ALL sets it
 * again).  A record whose fields do not fit inside it, or that is not the length its block_size says, is left as it is. */
PSSBAM_EM_FN void pssbam_end_mask_record(uint8_t *rec, uint32_t len, uint32_t mode, uint32_t n5, uint32_t n3)
{
    if (len < 36u || mode < PSSBAM_EM_ALL || mode > PSSBAM_EM_SS) return;
    const uint32_t block_size = pssbam_em_u32(rec), w12 = pssbam_em_u32(rec + 12), w16 = pssbam_em_u32(rec + 16), l = pssbam_em_u32(rec + 20);
    const uint32_t l_read_name = w12 & 0xFFu, n_cigar_op = w16 & 0xFFFFu, rev = (w16 >> 20) & 1u;   /* flag 0x10 */
    const uint64_t seq_at = 36ull + l_read_name + 4ull * n_cigar_op, qual_at = seq_at + ((uint64_t)l + 1ull) / 2ull;
    uint64_t have = 4ull + block_size;
    if (have > len) have = len;   /* (the index gives every record 4 + block_size bytes; should it not, the shorter one holds) */
    if (l == 0u || qual_at + l > have) return;
    uint8_t *seq = rec + seq_at, *qual = rec + qual_at;
    if (qual[0] == 0xFFu) qual = 0;   /* qualities absent: only SEQ is masked */
    const uint32_t k5 = n5 < l ? n5 : l, k3 = n3 < l ? n3 : l, kh = rev ? k3 : k5, kt = rev ? k5 : k3;
    const uint32_t strand_code = rev ? 1u : 8u;
    const uint32_t head_code = mode == PSSBAM_EM_ALL ? 0u : mode == PSSBAM_EM_DS ? 8u : strand_code;
    const uint32_t tail_code = mode == PSSBAM_EM_ALL ? 0u : mode == PSSBAM_EM_DS ? 1u : strand_code;
    pssbam_em_range(seq, qual, 0u, kh, head_code);
    pssbam_em_range(seq, qual, l - kt, l, tail_code);
}

#if defined(__HIPCC__)
namespace pssbam {

// A lane per input record of the block, as select_mark: dst is the scanned len[] (n + 1 entries), record r is kept iff
// dst[r + 1] > dst[r] and its copy then starts at out + dst[r]; out_bytes bounds the output (the block's own size).  The trip
// counts of the two walks are min(n5, l) and min(n3, l) bytes halved: the same in every lane but for reads shorter than the
// widths, so the wave does not wait for a long lane; what diverges is which lanes are kept, and a dropped lane costs two loads.
// The header loads of neighbouring lanes are a record apart (a few hundred bytes), the price of reading the output copy.
__global__ void __launch_bounds__(256) select_mask_ends(uint8_t *out, const uint32_t *dst, uint32_t n, uint64_t out_bytes, uint32_t mode,
                                                       uint32_t n5, uint32_t n3) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t r64 = blockIdx.x * blockDim.x + threadIdx.x; r64 < n; r64 += stride) {
        const uint32_t r = (uint32_t)r64, d0 = dst[r], d1 = dst[r + 1u];
        if (d1 <= d0 || d1 > out_bytes) continue;
        pssbam_end_mask_record(out + d0, d1 - d0, mode, n5, n3);
    }
}

}  // namespace pssbam
#endif

#endif

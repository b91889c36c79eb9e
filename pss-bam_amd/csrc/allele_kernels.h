// pss-bam_amd/csrc/allele_kernels.h -- strand-split allele counts of the kept records at listed sites (pssbam_engine_set_sites,
// pss-bam -a / -t).
//
// The resolved sites are 64-bit genome indices lo(contig) + p -- the indexing of P.genome and of coverage_add -- sorted ascending,
// sites[0, n) with one closing entry sites[n] = 2^64 - 1.  A lookup grid goes with them: grid[c] = the index of the first site at or
// after genome index c << shift, one word per 2^shift indices and one closing word = n, so that grid[c] .. grid[c + 1] bounds the
// sites of cell c.  Counters: uint32 counts[n][10] = fA fC fG fT fO rA rC rG rT rO, exact below 2^32.
//
//   allele_add       lane per record, behind the block's tally kernels (where coverage_add goes): the decision of select_keep, then
//                    for the record's window [a + t, b - t) one grid lookup (the cell's two adjacent words), a binary search inside
//                    the cell for the first site at or after the lower bound, and a walk over the sites below the upper bound.  Per
//                    hit: one nibble of SEQ, the QUAL byte under -Q, and one relaxed agent-scope atomic add whose result is not used.
//                    No lane waits on another, no LDS.  A record that meets no site -- nearly every record of a sparse panel --
//                    costs the two grid words and one or two site loads and never touches its SEQ or QUAL.
//   allele_ref_base  at finish, lane per site: the genome's stored base as a letter, A C G T, anything else N.
#pragma once

#include "coverage_kernels.h"

namespace pssbam {

static constexpr uint32_t ALLELE_CODES = 5, ALLELE_WORDS = 2 * ALLELE_CODES;   // A C G T other, forward then reverse

// sites has n + 1 entries, grid n_cells + 1, counts n * ALLELE_WORDS.  A kept
// record lies inside its contig, so its cell is one the grid has: the bound on the cell is there only so that a wrong reference
// table cannot make the kernel read outside the grid.  Every index into sites is at most n and every counter index below n *
// ALLELE_WORDS by construction (grid words are at most n; the walk stops at the closing entry).
__global__ void __launch_bounds__(256) allele_add(const TallyParams P, const uint64_t *sites, uint32_t n, const uint32_t *grid, uint64_t n_cells,
                                                  uint32_t shift, uint32_t trim, uint32_t *counts) {
    const uint32_t n_recs = select_n_recs(P);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t r64 = blockIdx.x * blockDim.x + threadIdx.x; r64 < n_recs; r64 += stride) {
        GappedPlan pl;
        RecHdr h;
        uint32_t rec_len;
        if (!select_keep(P, (uint32_t)r64, pl, rec_len, h)) continue;
        if (2ull * trim >= pl.L) continue;
        const uint64_t a0 = pl.gbase + (uint64_t)(uint32_t)pl.s, a = a0 + trim, b = a0 + pl.L - trim;
        const uint64_t c = a >> shift;
        if (c >= n_cells) continue;
        uint32_t lo = min(grid[c], n), hi = min(grid[c + 1], n);
        while (lo < hi) {   // the first site of the cell at or after a; hi (the first site of the cells behind it) when none is
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (sites[mid] < a) lo = mid + 1u;
            else hi = mid;
        }
        uint64_t v = sites[lo];
        if (v >= b) continue;
        GlobalBytes src{P.recs + P.offs[(uint32_t)r64]};
        uint32_t *const mine = counts + (pl.rev ? ALLELE_CODES : 0u);
        do {
            const uint32_t off = (uint32_t)(v - a0);   // < L
            uint32_t code = nib_code(read_nibble(src, h, off));   // (an offset at or beyond l_seq reads as nibble 0: other)
            if (P.min_bq && off < h.l_seq && src.u8(h.qual_off + off) < P.min_bq) code = 4u;   // (absent QUAL is 0xFF: never below)
            coverage_atomic_add(mine + (uint64_t)lo * ALLELE_WORDS + code, 1u);
            v = sites[++lo];   // (lo <= n: the closing entry ends the walk)
        } while (v < b);
    }
}

__global__ void __launch_bounds__(256) allele_ref_base(const uint8_t *genome, uint64_t genome_len, const uint64_t *sites, uint32_t n, uint8_t *out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint64_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const uint64_t at = sites[k];
        const uint32_t stored = at < genome_len ? genome[at] : 4u;
        out[k] = stored < 4u ? (uint8_t)((0x54474341u >> (8u * stored)) & 0xFFu) : (uint8_t)'N';   // "ACGT"
    }
}

}  // namespace pssbam

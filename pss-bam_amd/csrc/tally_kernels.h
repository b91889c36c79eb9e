// pss-bam_amd/csrc/tally_kernels.h -- the gfx950 tally kernels.
//
//  tally_simple : lane-per-read, records and reference bases gathered straight from
//                 global memory, counts into an LDS table (or global atomics when the
//                 table would not fit).  Any -r N, any k.  Cross-check of tally_tiled.
//  tally_tiled  : the production kernel.  One launch tallies 32 table rows (N <= 30: all of
//                 them; a larger -r takes one launch per 32 rows).  Persistent workgroups walk tiles
//                 of T = 128 consecutive reads:
//                   1. STAGE   LDS-DMA (global_load_lds_dwordx4) with a PER-LANE source address:
//                              lane q of the tile's piece list fetches 16-byte piece q % P of
//                              record q / P, and the hardware packs the pieces of one
//                              wave-instruction contiguously in LDS -- so record j's first
//                              P*16 bytes (header, name, CIGAR, SEQ, QUAL[0]: everything the
//                              path reads) land densely at stage + j*P*16.  The ~150 QUAL bytes
//                              of a 150-bp record are never requested: the staging buffer is
//                              half of a whole-record tile (4 workgroups per CU instead of 3)
//                              and half the DMA issue slots are saved -- HBM itself still moves
//                              whole 128-byte lines, so its traffic stays close to the record
//                              size -- and consecutive lanes read consecutive addresses (cheap
//                              for the texture addresser).  The next tile's DMA is issued as
//                              soon as CODES-A is done with the buffer.
//                   2. CODES   a lane pair per read (one lane per alignment end).  Part A:
//                              decode + filters from LDS, the end's reference window
//                              (32 bytes) and k-mer window gathered from the device genome,
//                              SEQ nibbles into registers.  Part B: one byte per window
//                              position = (cell << 1 | table) or a "no count" code, four
//                              positions per VALU instruction through v_perm_b32 used as a
//                              byte table (no memory lookups), written as the read's row of
//                              the code sheet.
//                   3. COLUMNS wave-per-read, lane = column of the code sheet: each lane
//                              owns one (end, position) and bumps ITS word of a
//                              [cell,table][row] LDS table.  Lanes of one wave-instruction
//                              never share a word and the two 32-lane halves hit disjoint
//                              banks, so the AA/CC/GG/TT skew of real data causes no
//                              serialisation at all.
//                 Counters leave LDS once, at kernel end, as plain stores into the workgroup's
//                 slot of a scratch buffer; reduce_partials sums the slots into the u64 block.
//
//  tally_tiled_planes / tally_simple_planes<PLANES> (-G, -S, -C): the same kernels with one table plane
//                 per read group (PLANES_RG: record -> plane by its first RG:Z value,
//                 read_group_plane), per fragment-length bin (PLANES_LEN: by Plan::L,
//                 length_bin_plane) or per contig set (PLANES_REF: by Plan::ref_plane, packed into
//                 the ref_info entry plan_head loads anyway); -S and -C stage prefixes as without planes.
//                 -J: per read-name replicate (PLANES_HASH: by read_name_replicate, a hash of the staged name); prefixes too.
//  tally_tiled_planes / tally_simple_planes<PLANES_EACH> (-A): one plane per BAM reference, any number of them.  A workgroup
//                 holds a few planes in LDS, owned by the refIDs its tiles meet (claimed in CODES-A, kept across tiles); a
//                 read that finds every slot taken is tallied by one lane straight into its plane of the counter block, and
//                 held planes leave LDS with 64-bit atomics into theirs (tally_tiled_body, PLANES_EACH).
//  tally_tiled_kmer_planes / tally_simple_kmer_planes<PLANES> (fragkon -G, -S, -C): the k-mer tally with one
//                 [k5 | k3] pair of 4^k bins per plane; the length selector reads Plan::Lk (what fragkon's -l / -L
//                 compare).  k <= KMER_LDS_MAX_K: one 2 * 4^k-word LDS histogram per plane slot of the launch;
//                 larger k: global 64-bit atomics straight into the plane's bins.
//
//  REGIONS twins of the three tiled kernels (-T): every candidate's alignment is looked up in the region table
//                 (record_decode.h: region_grid_load / region_resolve) in CODES-A; a read that meets no region is
//                 filtered.  The lane-per-read kernels do the same in make_plan when the table pointer is set.
//
//  HIST arm of tally_tiled (-H, pass 0 only): the fragment-length histogram of the reads that were added to the
//                 tables, from the registers that hold the decision anyway (Plan::L, pss_fwd / pss_rev).  Equal
//                 lengths are merged inside the wave first, the first HIST_LDS_MAX_BINS bins of each array live in
//                 LDS behind the staging buffer and leave it once, at kernel end (hist_wave_add below).
//
//  GAPPED arm of tally_tiled (-I, every pass): clipped and gapped reads by their anchored ends.  plan_head walks the CIGAR in
//                 the staged prefix (record_decode.h: cigar_anchor), a lane's read stream starts at its end's anchor and
//                 CODES-B blanks what lies outside the end's matched run; the reference side is the plain kernel's.
//
//  SCORE arm of tally_tiled (-y / -Y, pass 0 of a one-pass launch): a sum of caller-supplied weights over the C and G sites of the
//                 whole read, by distance from the read's ends and base quality (read_score is the definition, one lane per read;
//                 read_score_staged the pair's two halves in CODES-A); a read below the minimum stops being a candidate, and the
//                 histogram of the score lives in LDS behind the staging buffer.
//
//  MISM arm of tally_tiled (-n / -N / -V, pass 0 of a one-pass launch): the mismatch count of the whole read against the reference.
//                 The two lanes of a read's pair each compare one half of it in CODES-A, eight bases per step and nibble-parallel
//                 (count_mismatches_staged: SEQ from the staged prefix, the reference from the 4-bit genome image), and add
//                 their halves; a read beyond the limit stops being a candidate, and the histogram of min(m, M + 1) lives in
//                 LDS behind the staging buffer (mism_wave_add).  count_mismatches is the definition, one lane per read.
//
//  INTERIOR arm of tally_tiled (-W, pass 0 of a one-pass launch): the 4 x 4 substitution table of the read interior, every position
//                 at least d bases from both ends of a read that is added to a table.  The MISM arm's walk with another
//                 reduction (walk_read_staged is what the two share): each lane of a read's pair counts one half of the
//                 interior into 16 bins (count_interior_staged), keeps them as 16-bit pairs across the barriers until -U/-D
//                 have decided the read's fate, and the 17 words [table | reads] live in LDS behind the staging buffer
//                 (interior_wave_add).  count_interior is the definition, one lane per read.
//
//  COMP arm of tally_tiled (-P, pass 0 of a one-pass launch): the reference base composition w bases on either side of the 5' end of
//                 the reads in the forward table and of the 3' end of those in the reverse table.  The end's own window holds the
//                 inside half; the outside half is one more five-dword gather per candidate end, issued with the window's.  In
//                 CODES-B every lane turns the 64 nibbles around its end into classes in offset order, and the wave merges them
//                 per offset with five ballots into ten scalar counts that ten lanes add to [c5 | c3] in LDS behind the
//                 staging buffer (composition_wave_add).  count_composition is the definition, one lane per read.
//
// Integer/byte work only: no MFMA anywhere (the bound is HBM bandwidth).
#pragma once

#include "record_decode.h"

namespace pssbam {

constexpr int TILED_THREADS = 256;
constexpr int TILED_WAVES = TILED_THREADS / 64;
constexpr int TILED_ROWS = 32;         // table rows (window positions per end) one pass covers; a larger
                                       // N+2 takes several passes over the block, 32 rows each (row_base)
constexpr int KMER_LDS_MAX_K = 4;      // 2 * 4^4 * 4 B = 2 KiB of LDS
constexpr uint32_t STAGE_SLACK = 64;   // readable bytes behind a staging buffer
constexpr uint32_t CODE_NONE = 32;     // sheet byte meaning "no count"; every code >= 32 is one
constexpr uint32_t TABLE_WORDS = 64 * 32;  // codes 0..31 = (cell << 1) | table, 32..63 = trash bin
// per-workgroup partial results of tally_tiled in global scratch: [table 1024 | k-mer bins 512 | stat deltas 16]
constexpr uint32_t SCRATCH_KMER = 1024, SCRATCH_DELTA = 1536, SCRATCH_WORDS = 1552;
// -X (SITE): the in-context table behind a slot: [(read base << 2) | (reference G ? 2 : 0) | table][row], 16 x 32 words --
// an in-context cell always has reference base C or G (in table coordinates too: complementing swaps the two)
constexpr uint32_t SITE_WORDS = 16 * 32, SITE_SCRATCH_WORDS = SCRATCH_WORDS + SITE_WORDS;
constexpr uint32_t CODE_SITE = 64;     // sheet bit "the reference position is in context" (SITE instantiations only)
// -E (END): the conditional tables of a workgroup live in dynamic LDS as [(cell << 1) | table][N + 2 rows] words with the four
// read counters behind them; in a scratch slot they follow the plain words as [(cell << 1) | table][32 rows]
constexpr uint32_t END_SCRATCH_WORDS = SCRATCH_WORDS + 32 * 32;
constexpr uint32_t CODE_END = 64;      // sheet bit "the read's other end is marked" (END instantiations only)
__host__ __device__ inline uint32_t end_lds_bytes(uint32_t rows) { return (32u * rows + 4u) * 4u; }
constexpr uint32_t REF_LDS_ENTRIES = 64;   // BAM references whose contig info is cached in LDS (+1 for "*")

// ---------------------------------------------------------------------------------------
// per-read tally, lane-per-read form (tally_simple, and tile-overflow records)
// ---------------------------------------------------------------------------------------
struct LdsTableRowMajor {  // [table][row][16] u32 in LDS
    uint32_t *t;
    uint32_t rows;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        atomicAdd(&t[(table * rows + row) * 16u + cell], 1u);
    }
};
struct LdsTableColumnMajor {  // [(cell << 1) | table][32 rows] u32 in LDS (tiled kernel): rows row_base .. +31
    uint32_t *t;
    uint32_t row_base;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        const uint32_t r = row - row_base;
        if (r < 32u) atomicAdd(&t[(((cell << 1) | table) << 5) + r], 1u);
    }
};
struct GlobalTable {  // straight into the u64 counter block
    unsigned long long *c;
    uint32_t off_rev;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        atomicAdd(&c[(table ? off_rev : 0u) + row * 16u + cell], 1ull);
    }
};

// -X: where the lane-per-read form adds an in-context position a second time (NoSite: nowhere, the option is off)
struct NoSite {
    __device__ __forceinline__ void add(uint32_t, uint32_t, uint32_t) const {}
};
__device__ __forceinline__ uint32_t site_half_code(uint32_t table, uint32_t cell) {   // cell = 4 * read + reference, reference C or G
    return ((cell >> 2) << 2) | (cell & 2u) | table;
}
struct LdsSiteColumnMajor {  // the tiled kernel's [half code][32 rows] table of the rows row_base .. +31
    uint32_t *t;
    uint32_t row_base;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        const uint32_t r = row - row_base;
        if (r < 32u) atomicAdd(&t[(site_half_code(table, cell) << 5) + r], 1u);
    }
};
struct GlobalSite {  // straight into the [fwd_in | rev_in] pair of the counter block
    unsigned long long *c;
    uint32_t off_rev;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        atomicAdd(&c[(table ? off_rev : 0u) + row * 16u + cell], 1ull);
    }
};
// CpG context of contig position p from the stored genome bytes (C = 1, G = 2; anything else, padding included, is "no")
__device__ __forceinline__ bool site_in_cpg(const uint8_t *G, int64_t p) {
    const uint32_t b = G[p];
    return (b == 1u && G[p + 1] == 2u) || (b == 2u && G[p - 1] == 1u);
}

// One end of one read into one table.  `left` selects the alignment's left end
// (reference s-2.., read bases 0..) or right end (reference ..s+L+1, read bases ..L-1);
// `comp` complements both bases (reverse-strand reads), which maps cell c to 15-c.
// Restates add_ctx_counts + add_fwd_counts / add_rev_counts, pss-bam.c:169-326.
// MASKQ (-Q): a position whose read base has a QUAL byte below min_bq adds nothing, as if SEQ held 'N' there
// (add_fwd_counts / add_rev_counts skip every read base that is not A/C/G/T); the context rows are
// reference-only and never masked.  min_bq == 0 masks nothing.
// SITE (-X cpg): a position that is counted and whose reference position is in CpG context is added to `site` as well
// (genome orientation for both strands: the set is its own reverse complement); the context rows never are.
// GAPPED (-I): the read-side anchors of the record (GappedPlan::q0 / q1 / a / b); the reference side (s, L) stays as it is.  A
// position counts when no I / D lies between it and one of the alignment's two ends: reference offset g < a is read base q0 + g (the
// run at the start), g >= L - b is read base q1 - (L - g) (the run at the end, which a window longer than L - b reaches from the
// far side), anything between adds nothing, like an N.  Without GAPPED the read index is the reference offset, as for every <len>M
// record.
struct ReadAnchors { uint32_t q0, q1, a, b; };
struct NoAnchors {};   // (an empty argument: the instantiations without GAPPED keep their signature)
template <bool MASKQ, bool SITE, bool GAPPED = false, class Src, class Tab, class Site, class An = NoAnchors>
__device__ void tally_end(const Tab &tab, const Site &site, uint32_t table, const Src &src, const RecHdr &h, const uint8_t *G,
                          int64_t s, uint32_t L, int N, bool left, bool comp, uint32_t min_bq, An an = An{}) {
    const uint32_t c0 = ref_code(left ? G[s - 2] : G[s + L + 1]);  // second context base -> row 0
    const uint32_t c1 = ref_code(left ? G[s - 1] : G[s + L]);      // first context base  -> row 1
    if (c0 < 4u) tab.add(table, 0, comp ? 15u - 5u * c0 : 5u * c0);
    if (c1 < 4u) tab.add(table, 1, comp ? 15u - 5u * c1 : 5u * c1);
    for (int i = 0; i < N; i++) {
        const uint32_t gi = left ? (uint32_t)i : L - 1u - (uint32_t)i;   // offset of the position in the alignment's reference stretch
        uint32_t ri = gi;
        if constexpr (GAPPED) {
            if (gi < an.a) ri = an.q0 + gi;
            else if (gi >= L - an.b) ri = an.q1 - (L - gi);
            else continue;                                               // between the two runs
        }
        if (MASKQ && ri < h.l_seq && src.u8(h.qual_off + ri) < min_bq) continue;   // (absent QUAL is 0xFF: never below)
        const uint32_t rd = nib_code(read_nibble(src, h, ri));
        const uint32_t rf = ref_code(G[s + (int64_t)gi]);
        if (rd < 4u && rf < 4u) {
            const uint32_t cell = 4u * rd + rf;
            tab.add(table, (uint32_t)i + 2u, comp ? 15u - cell : cell);
            if constexpr (SITE) {
                if (site_in_cpg(G, s + (int64_t)gi)) site.add(table, (uint32_t)i + 2u, comp ? 15u - cell : cell);
            }
        }
    }
}

template <bool MASKQ = false, bool SITE = false, bool GAPPED = false, class Src, class Tab, class Site>
__device__ __forceinline__ void tally_pss_record(const TallyParams &P, const Tab &tab, const Site &site, const Src &src,
                                                 const RecHdr &h, const typename PlanOf<GAPPED>::type &pl) {
    const uint32_t min_bq = MASKQ ? P.min_bq : 0u;
    const uint8_t *G = P.genome + pl.gbase;
    // forward-strand read: fwd table <- left end, rev table <- right end;
    // reverse-strand read: fwd table <- right end complemented, rev table <- left end complemented
    if constexpr (GAPPED) {   // (a plan made by the GAPPED plan_head)
        const ReadAnchors an{pl.q0, pl.q1, pl.a, pl.b};
        if (pl.pss_fwd) tally_end<MASKQ, SITE, true>(tab, site, 0u, src, h, G, pl.s, pl.L, P.N, !pl.rev, pl.rev, min_bq, an);
        if (pl.pss_rev) tally_end<MASKQ, SITE, true>(tab, site, 1u, src, h, G, pl.s, pl.L, P.N, pl.rev, pl.rev, min_bq, an);
    } else {
    if (pl.pss_fwd) tally_end<MASKQ, SITE>(tab, site, 0u, src, h, G, pl.s, pl.L, P.N, !pl.rev, pl.rev, min_bq);
    if (pl.pss_rev) tally_end<MASKQ, SITE>(tab, site, 1u, src, h, G, pl.s, pl.L, P.N, pl.rev, pl.rev, min_bq);
    }
}
template <bool MASKQ = false, class Src, class Tab>
__device__ __forceinline__ void tally_pss_record(const TallyParams &P, const Tab &tab, const Src &src,
                                                 const RecHdr &h, const Plan &pl) {
    tally_pss_record<MASKQ, false>(P, tab, NoSite{}, src, h, pl);
}

// -E: is one end of a read marked -- does one of its first `depth` positions carry the cell `want` (table coordinates,
// the cell tally_end would add at row 2 + i)?  left / comp as in tally_end; a base masked by -Q has no cell.
template <bool MASKQ, class Src>
__device__ bool end_marked(const Src &src, const RecHdr &h, const uint8_t *G, int64_t s, uint32_t L, uint32_t depth, bool left,
                           bool comp, uint32_t min_bq, uint32_t want) {
    for (uint32_t i = 0; i < depth; i++) {
        const uint32_t ri = left ? i : L - 1u - i;
        if (MASKQ && ri < h.l_seq && src.u8(h.qual_off + ri) < min_bq) continue;
        const uint32_t rd = nib_code(read_nibble(src, h, ri));
        const uint32_t rf = ref_code(G[s + (int64_t)ri]);
        if (rd < 4u && rf < 4u && (comp ? 15u - (4u * rd + rf) : 4u * rd + rf) == want) return true;
    }
    return false;
}
struct LdsEndTable {  // the tiled kernel's [(cell << 1) | table][rows] conditional tables, reads[4] behind them
    uint32_t *t;
    uint32_t rows;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        atomicAdd(&t[((cell << 1) | table) * rows + row], 1u);
    }
    __device__ __forceinline__ void count(uint32_t k) const { atomicAdd(&t[32u * rows + k], 1u); }
};
struct GlobalEndTable {  // straight into [fwd_c | rev_c | reads[4]] of the counter block
    unsigned long long *c;
    uint32_t off_rev;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        atomicAdd(&c[(table ? off_rev : 0u) + row * 16u + cell], 1ull);
    }
    __device__ __forceinline__ void count(uint32_t k) const { atomicAdd(&c[2u * off_rev + k], 1ull); }
};
// -E, lane-per-read form: an unpaired record that was added to the tables is counted in reads[], its forward contribution
// is added to `cond` a second time when its 3' end is marked, its reverse contribution when its 5' end is (the forward
// table is fed from the 5' end: the left alignment end of a forward read, the complemented right end of a reverse read)
template <bool MASKQ, class Src, class Cond>
__device__ __forceinline__ void tally_end_condition(const TallyParams &P, const Cond &cond, const Src &src, const RecHdr &h, const Plan &pl) {
    if ((pl.flag & FL_PAIRED) || !(pl.pss_fwd && pl.pss_rev)) return;
    const uint32_t min_bq = MASKQ ? P.min_bq : 0u;
    const uint8_t *G = P.genome + pl.gbase;
    const bool m5 = end_marked<MASKQ>(src, h, G, pl.s, pl.L, P.end_depth, !pl.rev, pl.rev, min_bq, P.end_cell5);
    const bool m3 = end_marked<MASKQ>(src, h, G, pl.s, pl.L, P.end_depth, pl.rev, pl.rev, min_bq, P.end_cell3);
    cond.count(0u);
    if (m5) cond.count(1u);
    if (m3) cond.count(2u);
    if (m5 && m3) cond.count(3u);
    if (m3) tally_end<MASKQ, false>(cond, NoSite{}, 0u, src, h, G, pl.s, pl.L, P.N, !pl.rev, pl.rev, min_bq);
    if (m5) tally_end<MASKQ, false>(cond, NoSite{}, 1u, src, h, G, pl.s, pl.L, P.N, pl.rev, pl.rev, min_bq);
}

// one k-mer add (5' when which == 0, 3' when which == 1); false = non-ACGT in the window
template <bool LDS_KMER>
__device__ __forceinline__ bool tally_one_kmer(const TallyParams &P, const Plan &pl, uint32_t which, uint32_t *lds_kmer) {
    const uint8_t *G = P.genome + pl.gbase;
    int64_t w5, w3;
    kmer_windows(pl, P.K, w5, w3);
    uint32_t bin;
    if (!kmer_bin(G, which ? w3 : w5, P.K, pl.rev, bin)) return false;
    if (LDS_KMER) atomicAdd(&lds_kmer[(which ? (1u << (2 * P.K)) : 0u) + bin], 1u);
    else atomicAdd(&P.counters[(which ? P.off_k3 : P.off_k5) + bin], 1ull);
    return true;
}

// both k-mer adds of one record; true = an attempted add failed (fragkon's status -1)
// (fragkon.c:164-181: both attempted, 0 only if both succeeded; :198-210 single add)
template <bool LDS_KMER>
__device__ __forceinline__ bool tally_kmer_record(const TallyParams &P, const Plan &pl, uint32_t *lds_kmer) {
    bool good = true;
    if (pl.fk5) good = tally_one_kmer<LDS_KMER>(P, pl, 0u, lds_kmer) && good;
    if (pl.fk3) good = tally_one_kmer<LDS_KMER>(P, pl, 1u, lds_kmer) && good;
    return !good;
}

// ---------------------------------------------------------------------------------------
// -H: fragment-length histogram of the reads added to the forward / reverse table
// ---------------------------------------------------------------------------------------
// hf / hr of the counter block hold hist_max + 2 bins each (bin hist_max + 1 = "longer").  The tiled kernel keeps bins
// 0 .. hist_lds_bins - 1 of both arrays as u32 words in LDS, [hf | hr]; hist_lds_bins = min(hist_max + 2,
// HIST_LDS_MAX_BINS), i.e. at most 8 KiB, which every limit up to 1022 fits whole.  Bins beyond that (a limit above
// 1022 AND a read that long) go to the counter block with 64-bit atomics, merged inside the wave first.
constexpr uint32_t HIST_LDS_MAX_BINS = 1024;
__host__ __device__ inline uint32_t hist_lds_bytes(uint32_t lds_bins) { return 2u * lds_bins * 4u; }

// n reads of bin b into hf (fwd) and / or hr (rev)
__device__ __forceinline__ void hist_add(const TallyParams &P, uint32_t *hist_lds, uint32_t b, bool fwd, bool rev, uint32_t n) {
    if (b < P.hist_lds_bins) {
        if (fwd) atomicAdd(&hist_lds[b], n);
        if (rev) atomicAdd(&hist_lds[P.hist_lds_bins + b], n);
    } else {
        if (fwd) atomicAdd(&P.counters[P.off_hist + b], (unsigned long long)n);
        if (rev) atomicAdd(&P.counters[P.off_hist + P.hist_max + 2u + b], (unsigned long long)n);
    }
}
__device__ __forceinline__ uint32_t hist_bin(const TallyParams &P, uint32_t L) { return min(L, P.hist_max + 1u); }

// The whole wave's reads of one tile (called from uniform control flow; `on` = this lane holds a read that was added
// to a table).  A modern library puts every read of the wave in ONE bin and an ancient-DNA library in a few dozen, so
// lanes are merged by value before anything is added: the lanes that hold the first pending lane's (bin, fwd, rev)
// are counted with one ballot and their leader adds the count once.  Two such rounds take the modes of the
// distribution; what is left after them is spread thin, and for a bin that lives in LDS a lane's own add is then
// cheaper than another round (an LDS atomic whose lanes meet on a word costs a cycle per lane, nothing more).  Bins
// that live in the counter block are merged to the end: a wave sends at most one global atomic per distinct bin.
__device__ __forceinline__ void hist_wave_add(const TallyParams &P, uint32_t *hist_lds, bool on, uint32_t L, bool fwd, bool rev) {
    const uint32_t b = hist_bin(P, L);
    const uint32_t key = (b << 2) | (fwd ? 2u : 0u) | (rev ? 1u : 0u);
    const uint32_t lane = threadIdx.x & 63u;
    bool pending = on && (fwd || rev);
    for (uint32_t round = 0; __any(pending); round++) {
        if (pending) {
            if (round >= 2u && b < P.hist_lds_bins) {
                hist_add(P, hist_lds, b, fwd, rev, 1u);
                pending = false;
            } else {
                const uint32_t v = __builtin_amdgcn_readfirstlane(key);   // (of the lanes still in this branch)
                const bool same = key == v;
                const unsigned long long m = __ballot(same);
                if (same) {
                    pending = false;
                    if (lane == (uint32_t)__ffsll((long long)m) - 1u) hist_add(P, hist_lds, b, fwd, rev, (uint32_t)__popcll(m));
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// -n / -N / -V: mismatches of a whole read against the reference
// ---------------------------------------------------------------------------------------
// The mismatch count m of a <L>M record (include/pssbam_hip.h): the read positions i < min(L, l_seq) at which both SEQ[i] and the
// reference base are one of A C G T and differ -- with tv_only, differ by a transversion (stored codes A0 C1 G2 T3: a transition
// is an XOR of 2).  Strand-independent; -Q does not enter.  This is the definition in code: tally_simple and the one-lane
// path of tally_tiled use it as it stands.
template <class Src>
__device__ uint32_t count_mismatches(const Src &src, const RecHdr &h, const uint8_t *G, int64_t s, uint32_t L, bool tv_only) {
    const uint32_t n = min(L, h.l_seq);
    uint32_t m = 0u;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t rd = nib_code(read_nibble(src, h, i));
        const uint32_t rf = ref_code(G[s + (int64_t)i]);
        if (rd < 4u && rf < 4u && rd != rf && !(tv_only && (rd ^ rf) == 2u)) m++;
    }
    return m;
}
// TallyParams::mism_limit is k + 1 (0 = no filter), mism_hist the histogram limit M (0 = no histogram)
__device__ __forceinline__ bool mism_on(const TallyParams &P) { return (P.mism_hist | P.mism_limit) != 0u; }
__device__ __forceinline__ bool mism_beyond(const TallyParams &P, uint32_t m) { return P.mism_limit && m >= P.mism_limit; }
__device__ __forceinline__ uint32_t mism_bin(const TallyParams &P, uint32_t m) { return min(m, P.mism_hist + 1u); }
// n reads of bin b into mf (fwd) and / or mr (rev): the tiled kernel's LDS bins [mf | mr], or the counter block
__device__ __forceinline__ void mism_add(const TallyParams &P, uint32_t *mism_lds, uint32_t b, bool fwd, bool rev, uint32_t n) {
    if (mism_lds) {
        if (fwd) atomicAdd(&mism_lds[b], n);
        if (rev) atomicAdd(&mism_lds[P.mism_hist + 2u + b], n);
    } else {
        if (fwd) atomicAdd(&P.counters[P.off_mism + b], (unsigned long long)n);
        if (rev) atomicAdd(&P.counters[P.off_mism + P.mism_hist + 2u + b], (unsigned long long)n);
    }
}
// The whole wave's reads of one tile, merged by value like hist_wave_add (most reads of a wave have 0, 1 or 2 mismatches):
// two ballot rounds take the modes, what is left adds itself.  Every bin lives in LDS.  add(b, fwd, rev, n): n reads of bin b.
template <class Add>
__device__ __forceinline__ void bin_wave_add(bool on, uint32_t b, bool fwd, bool rev, Add add) {
    const uint32_t key = (b << 2) | (fwd ? 2u : 0u) | (rev ? 1u : 0u);
    const uint32_t lane = threadIdx.x & 63u;
    bool pending = on && (fwd || rev);
    for (uint32_t round = 0; __any(pending); round++) {
        if (pending) {
            if (round >= 2u) {
                add(b, fwd, rev, 1u);
                pending = false;
            } else {
                const uint32_t v = __builtin_amdgcn_readfirstlane(key);   // (of the lanes still in this branch)
                const bool same = key == v;
                const unsigned long long m = __ballot(same);
                if (same) {
                    pending = false;
                    if (lane == (uint32_t)__ffsll((long long)m) - 1u) add(b, fwd, rev, (uint32_t)__popcll(m));
                }
            }
        }
    }
}
__device__ __forceinline__ void mism_wave_add(const TallyParams &P, uint32_t *mism_lds, bool on, uint32_t b, bool fwd, bool rev) {
    bin_wave_add(on, b, fwd, rev, [&](uint32_t bin, bool f, bool r, uint32_t n) { mism_add(P, mism_lds, bin, f, r, n); });
}
// Eight positions at once.  g: eight nibbles of the genome image (0..3 = A C G T, 4..7 = other), r: the BAM nibbles of the
// same eight read bases in the same order.  Returns bit 4q set when position q counts.  The reference nibble becomes the BAM
// one-hot code (1 2 4 8), so the XOR of the two is zero for a match, 5 (A/G) or 10 (C/T) for a transition; a read nibble is
// a base when exactly one of its bits is set.
__device__ __forceinline__ uint32_t nonzero_nibbles8(uint32_t y) { return (y | (y >> 1) | (y >> 2) | (y >> 3)) & 0x11111111u; }   // bit 0 of every nibble that is not 0
// bit 4q set when position q holds one of A C G T on both sides: a reference nibble below 4, a read nibble with exactly one bit
__device__ __forceinline__ uint32_t acgt_pair_flags8(uint32_t g, uint32_t r) {
    const uint32_t K = 0x11111111u;
    const uint32_t g_ok = ~(g >> 2) & ~(g >> 3) & K;
    const uint32_t bits = (r & K) + ((r >> 1) & K) + ((r >> 2) & K) + ((r >> 3) & K);   // 0..4 per nibble: no carry
    const uint32_t r_ok = ~nonzero_nibbles8(bits ^ K) & K;
    return g_ok & r_ok;
}
__device__ __forceinline__ uint32_t mismatch_flags8(uint32_t g, uint32_t r, bool tv_only) {
    const uint32_t K = 0x11111111u;
    const uint32_t g0 = g & K, g1 = (g >> 1) & K;
    const uint32_t onehot = (~g1 & ~g0 & K) | ((~g1 & g0) << 1) | ((g1 & ~g0) << 2) | ((g1 & g0) << 3);
    const uint32_t ok = acgt_pair_flags8(g, r);
    const uint32_t x = r ^ onehot;
    uint32_t f = ok & nonzero_nibbles8(x);
    if (tv_only) f &= nonzero_nibbles8(x ^ 0x55555555u) & nonzero_nibbles8(x ^ 0xAAAAAAAAu);
    return f;
}

// ---------------------------------------------------------------------------------------
// -y / -Y: a weighted score over the C and G sites of a whole read
// ---------------------------------------------------------------------------------------
// The score S of a <L>M record (include/pssbam_hip.h): over the read positions i < min(L, l_seq) at which SEQ[i] and the reference base
// are both one of A C G T and, under -Q, QUAL[i] is not below the minimum, the sum of weights[kind][d][q] -- reference C against read
// C / T is kind 0 / 1 at d = i, reference G against read G / A kind 2 / 3 at d = L - 1 - i, a FLAG 0x10 record swaps 0 1 with 2 3, d and
// q = QUAL[i] saturate at the table's last row and column, every other pair adds nothing.  Stored codes A0 C1 G2 T3.  This is the
// definition in code: tally_simple and the one-lane path of tally_tiled use it as it stands; a record there may be longer than 2^20
// bases, hence the 64-bit sum.
template <class Src>
__device__ int32_t read_score(const TallyParams &P, const Src &src, const RecHdr &h, const uint8_t *G, int64_t s, uint32_t L, bool rev) {
    const uint32_t n = min(L, h.l_seq);
    long long S = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t rd = nib_code(read_nibble(src, h, i));
        const uint32_t rf = ref_code(G[s + (int64_t)i]);
        if (rd >= 4u || rf >= 4u) continue;
        const uint32_t qv = src.u8(h.qual_off + i);
        if (P.min_bq && qv < P.min_bq) continue;
        uint32_t kind, d;
        if (rf == 1u && (rd == 1u || rd == 3u)) { kind = rd == 3u ? 1u : 0u; d = i; }
        else if (rf == 2u && (rd == 2u || rd == 0u)) { kind = rd == 0u ? 3u : 2u; d = L - 1u - i; }
        else continue;
        if (rev) kind ^= 2u;
        S += P.score_w[(kind * P.score_nd + min(d, P.score_nd - 1u)) * P.score_nq + min(qv, P.score_nq - 1u)];
    }
    return (int32_t)max(-2147483647ll - 1ll, min(S, 2147483647ll));
}
__device__ __forceinline__ bool score_below(const TallyParams &P, int32_t S) { return P.score_filter && S < P.score_min; }
// bin clamp(S >> shift, -H, H - 1) + H: the shift is arithmetic, so it floors negative scores as well
__device__ __forceinline__ uint32_t score_bin(const TallyParams &P, int32_t S) {
    const int32_t H = (int32_t)P.score_half;
    return (uint32_t)(max(-H, min(S >> P.score_shift, H - 1)) + H);
}
// n reads of bin b into sf (fwd) and / or sr (rev): the tiled kernel's LDS bins [sf | sr], or the counter block
__device__ __forceinline__ void score_add(const TallyParams &P, uint32_t *score_lds, uint32_t b, bool fwd, bool rev, uint32_t n) {
    if (score_lds) {
        if (fwd) atomicAdd(&score_lds[b], n);
        if (rev) atomicAdd(&score_lds[2u * P.score_half + b], n);
    } else {
        if (fwd) atomicAdd(&P.counters[P.off_score + b], (unsigned long long)n);
        if (rev) atomicAdd(&P.counters[P.off_score + 2u * P.score_half + b], (unsigned long long)n);
    }
}

// ---------------------------------------------------------------------------------------
// -W: the substitution table of the read interior
// ---------------------------------------------------------------------------------------
// The interior of a record that is added to the forward or the reverse table (include/pssbam_hip.h): the read positions i with
// d <= i, i + d < L and i < l_seq, d = P.interior - 1.  A position counts when SEQ[i] and the reference base are both one of A C G T
// and, under -Q, QUAL[i] is not below the minimum (absent qualities are 0xFF: never below); it counts into bin 4 * read + ref of
// table[16], a reverse-strand record into 15 - that (both bases complemented), and a record whose interior is not empty
// counts once in `reads` (word 16).  This is the definition in code: tally_simple and the one-lane path of tally_tiled use it
// as it stands, and add straight into the counter block.
template <class Src>
__device__ void count_interior(const TallyParams &P, const Src &src, const RecHdr &h, const uint8_t *G, int64_t s, uint32_t L, bool rev) {
    const uint32_t d = P.interior - 1u;
    const uint32_t hi = L > d ? min(L - d, h.l_seq) : 0u;
    if (hi <= d) return;
    for (uint32_t i = d; i < hi; i++) {
        const uint32_t rd = nib_code(read_nibble(src, h, i));
        const uint32_t rf = ref_code(G[s + (int64_t)i]);
        if (rd >= 4u || rf >= 4u) continue;
        if (P.min_bq && src.u8(h.qual_off + i) < P.min_bq) continue;
        const uint32_t bin = 4u * rd + rf;
        atomicAdd(&P.counters[P.off_interior + (rev ? 15u - bin : bin)], 1ull);
    }
    atomicAdd(&P.counters[P.off_interior + 16u], 1ull);
}
constexpr uint32_t INTERIOR_WORDS = 17;   // table[16] | reads
// Eight positions at once, g and r as for mismatch_flags8, keep = the nibbles (all four bits) of the positions that belong to
// the lane's range and pass -Q.  Four read-letter planes against four reference-letter planes; a popcount of each AND is
// the step's share of a bin (v_bcnt adds it to the running count in the same instruction).
__device__ __forceinline__ void interior_step8(uint32_t g, uint32_t r, uint32_t keep, uint32_t (&cnt)[16]) {
    const uint32_t K = 0x11111111u;
    const uint32_t v = acgt_pair_flags8(g, r) & keep;
    const uint32_t g0 = g & K, g1 = (g >> 1) & K;
    const uint32_t rf[4] = {v & ~(g0 | g1), v & g0 & ~g1, v & g1 & ~g0, v & g0 & g1};
    const uint32_t rd[4] = {r & K, (r >> 1) & K, (r >> 2) & K, (r >> 3) & K};   // (one bit per valid nibble: BAM A 1, C 2, G 4, T 8)
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) cnt[4 * a + b] += (uint32_t)__popc(rd[a] & rf[b]);
}
// The lanes of one wave into the workgroup's 17 LDS words.  pk[k] holds this lane's counts of bins 2k (low half) and 2k + 1;
// `on` = the lane's read was added to a table, `read` = it is the lane that counts the read itself.  A reverse-strand lane
// turns its bins round (bin b -> 15 - b: the registers in reverse order, halves swapped), the lanes of every row of 16 are
// summed with four DPP adds per register -- 16 lanes of at most 2048 bases each stay inside 16 bits -- and one lane per
// row adds the non-zero bins: the four diagonal bins take nearly everything, so a wave sends a few dozen LDS atomics
// instead of a few hundred.  Called from uniform control flow.
__device__ __forceinline__ void interior_wave_add(uint32_t *lds, const uint32_t (&pk)[8], bool on, bool rev, bool read) {
    if (!__any(on)) return;
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t m = pk[7 - k];
        o[k] = !on ? 0u : rev ? (m >> 16) | (m << 16) : pk[k];
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        o[k] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)o[k], 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
        o[k] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)o[k], 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
        o[k] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)o[k], 0x141, 0xF, 0xF, false);   // row_half_mirror
        o[k] += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)o[k], 0x140, 0xF, 0xF, false);   // row_mirror
    }
    if ((threadIdx.x & 15u) == 0u) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (o[k] & 0xFFFFu) atomicAdd(&lds[2 * k], o[k] & 0xFFFFu);
            if (o[k] >> 16) atomicAdd(&lds[2 * k + 1], o[k] >> 16);
        }
    }
    const unsigned long long n = __ballot(on && read);
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(&lds[16], (uint32_t)__popcll(n));
}

// ---------------------------------------------------------------------------------------
// -P: the reference base composition around the read ends
// ---------------------------------------------------------------------------------------
// A record that is added to the forward table counts the 2w reference positions around its 5' end into c5, one that is added to
// the reverse table those around its 3' end into c3 (include/pssbam_hip.h): offset j = -w .. w - 1 from the end, negative outside the
// read, is position s + j at the alignment's left end and s + L - 1 - j at its right end; a forward-strand record has its 5' end on the
// left, a FLAG 0x10 record on the right, and the latter's classes are complemented.  class = 0 1 2 3 for A C G T, 4 for anything
// else; row j + w, five words per row.  A position counts only inside its contig (0 <= p < glen, glen = the contig's length), and an
// inside offset only below L: masked by position, whatever letter lies there.  This is the definition in code: tally_simple and the
// one-lane path of tally_tiled use it as it stands, and add straight into the counter block.
__device__ __forceinline__ uint32_t contig_length(const TallyParams &P, const RecHdr &h) {
    return P.ref_info[(uint32_t)h.ref_id < (uint32_t)P.n_ref ? (uint32_t)h.ref_id : (uint32_t)P.n_ref].z;
}
__device__ void count_composition(const TallyParams &P, const uint8_t *G, int64_t glen, int64_t s, uint32_t L, bool rev, bool fwd_table, bool rev_table) {
    const int32_t w = (int32_t)P.composition;
    for (uint32_t blk = 0; blk < 2u; blk++) {
        if (!(blk ? rev_table : fwd_table)) continue;
        const bool right = (blk != 0u) != rev;   // the 5' end of a forward-strand record and the 3' end of a reverse-strand one are on the left
        for (int32_t j = -w; j < w; j++) {
            if (j >= 0 && (uint32_t)j >= L) continue;
            const int64_t p = right ? s + (int64_t)L - 1 - j : s + j;
            if (p < 0 || p >= glen) continue;
            const uint32_t c = ref_code(G[p]);
            const uint32_t cls = rev && c < 4u ? 3u - c : c;
            atomicAdd(&P.counters[P.off_composition + (blk * 2u * (uint32_t)w + (uint32_t)(j + w)) * 5u + cls], 1ull);
        }
    }
}
constexpr uint32_t COMP_MAX_WORDS = 2u * 2u * 30u * 5u;   // [c5 | c3] at the largest width: 600 words

// Nibble q of the result = nibble 7 - q of x.
__device__ __forceinline__ uint32_t reverse_nibbles8(uint32_t x) {
    const uint32_t y = __builtin_bswap32(x);
    return ((y >> 4) & 0x0F0F0F0Fu) | ((y & 0x0F0F0F0Fu) << 4);
}
// How many lanes of the wave hold class X, those of the 5' block into lane X of v and those of the 3' block (in3) into lane 5 + X:
// the two counts are scalars, and v_writelane places a scalar in one lane of a vector register.
template <int X>
__device__ __forceinline__ void composition_class(uint32_t cls, unsigned long long in3, uint32_t &v) {
    const unsigned long long m = __ballot(cls == (uint32_t)X);
    const uint32_t n5 = (uint32_t)__popcll(m & ~in3), n3 = (uint32_t)__popcll(m & in3);
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(n5), "n"(X));
    asm("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(n3), "n"(5 + X));
}
// -P, tiled form: the lanes of one wave into the workgroup's [c5 | c3] words in LDS.  u[k] holds this lane's reference nibbles (packed
// reference: 0..3 = A C G T, anything else "other") of the offsets 8k - 32 .. 8k - 25 from its own alignment end, nibble q = offset
// 8k + q - 32: u[0..3] the 32 positions outside the read, the adjacent one last, u[4..7] the ones inside, the end's own base first.
// The lane counts the offsets j with lo <= j < hi (lo <= 0 <= hi; lo = hi = 0: nothing) into block `blk` (0 = c5, 1 = c3), complemented
// when `rev`.  Every nibble becomes its class (0..4; 15 where the lane does not count); per offset one ballot per class, split by
// block with the ballot of `blk`, gives the wave's ten counts as scalars, which ten lanes add to their own LDS words: 2w wave-wide
// LDS adds per tile and wave, no two lanes on one word.  Called from uniform control flow.
__device__ __forceinline__ void composition_wave_add(uint32_t *lds, uint32_t w, const uint32_t (&u)[8], int32_t lo, int32_t hi, uint32_t blk, bool rev) {
    const uint32_t K = 0x11111111u;
    const unsigned long long in3 = __ballot(blk != 0u);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t mine = lane < 10u ? (lane >= 5u ? 10u * w + lane - 5u : lane) : 0u;   // word of offset -w, this lane's block and class
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (8 * k + 8 <= 32 - (int32_t)w || 8 * k >= 32 + (int32_t)w) continue;   // (uniform: the width is a kernel argument)
        // classes: a nibble above 3 becomes 4, a base of a reverse-strand lane its complement
        const uint32_t other = ((u[k] >> 2) | (u[k] >> 3)) & K;
        const uint32_t base3 = (other ^ K) * 3u;
        uint32_t c = ((rev ? ~u[k] : u[k]) & base3) | (other << 2);
        // the offsets this lane counts: nibbles a .. b - 1 of this word
        const int32_t a_s = lo + 32 - 8 * k, b_s = hi + 32 - 8 * k;
        const uint32_t a = a_s <= 0 ? 0u : a_s >= 8 ? 8u : (uint32_t)a_s, b = b_s <= 0 ? 0u : b_s >= 8 ? 8u : (uint32_t)b_s;
        const uint32_t below_b = b >= 8u ? 0xFFFFFFFFu : (1u << (4u * b)) - 1u, below_a = a >= 8u ? 0xFFFFFFFFu : (1u << (4u * a)) - 1u;
        c |= ~(below_b & ~below_a);
        // the offsets of this word that the width covers (uniform); a rolled loop, one nibble a turn: the ten counts of an offset are
        // scalars, and nothing of a later offset is worth holding in registers meanwhile
        const int32_t q0 = max(0, 32 - (int32_t)w - 8 * k), q1 = min(8, 32 + (int32_t)w - 8 * k);
        c >>= 4 * q0;
#pragma unroll 1
        for (int32_t q = q0; q < q1; q++, c >>= 4) {
            const uint32_t cls = c & 15u;
            uint32_t v = 0u;
            composition_class<0>(cls, in3, v);
            composition_class<1>(cls, in3, v);
            composition_class<2>(cls, in3, v);
            composition_class<3>(cls, in3, v);
            composition_class<4>(cls, in3, v);
            if (lane < 10u && v) atomicAdd(&lds[mine + 5u * (uint32_t)(8 * k + q - 32 + (int32_t)w)], v);   // row j + w
        }
    }
}

// ---------------------------------------------------------------------------------------
// tally_simple
// ---------------------------------------------------------------------------------------
// dynamic LDS: [2*(N+2)*16 u32 table, if LDS_TABLE]
template <bool LDS_TABLE>
__global__ void __launch_bounds__(256) tally_simple(const TallyParams P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_lds[];
    __shared__ int32_t lds_delta[ST_USED];
    const uint32_t rows = (uint32_t)P.N + 2u;
    const uint32_t tab_words = LDS_TABLE ? 2u * rows * 16u : 0u;
    const bool do_pss = (P.tally_mask & 1u) != 0, do_kmer = (P.tally_mask & 2u) != 0;
    for (uint32_t i = threadIdx.x; i < tab_words; i += blockDim.x) dyn_lds[i] = 0u;
    if (threadIdx.x < ST_USED) lds_delta[threadIdx.x] = 0;
    __syncthreads();

    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < P.n_recs; r += stride) {
        const uint32_t o0 = P.offs[r], o1 = P.offs[r + 1];
        GlobalBytes src{P.recs + o0};
        const RecHdr h = decode_hdr(src, o1 - o0);
        GappedPlan pl;   // (-I: substitution tables only; without it the anchors stay unset and unread)
        if (P.gapped) pl = make_plan<true, false, true, true>(P, src, h);
        else static_cast<Plan &>(pl) = make_plan<true, true>(P, src, h);
        if (!do_pss) pl.pss_fwd = pl.pss_rev = false;
        if (!do_kmer) pl.fk5 = pl.fk3 = false;
        // -n / -N: the read's mismatch count; beyond the limit it is filtered like a read that meets no region
        uint32_t mm = 0u;
        if (mism_on(P) && (pl.pss_fwd || pl.pss_rev)) {
            mm = count_mismatches(src, h, P.genome + pl.gbase, pl.s, pl.L, P.mism_tv != 0u);
            if (mism_beyond(P, mm)) pl.pss_fwd = pl.pss_rev = false;
        }
        // -y / -Y: the read's score; below the minimum it is filtered in the same way
        int32_t sc = 0;
        if (P.score_w && (pl.pss_fwd || pl.pss_rev)) {
            sc = read_score(P, src, h, P.genome + pl.gbase, pl.s, pl.L, pl.rev);
            if (score_below(P, sc)) pl.pss_fwd = pl.pss_rev = false;
        }
        if (pl.pss_fwd || pl.pss_rev) {
            if (P.gapped) {   // -I (never together with -X, -E or -H)
                if (LDS_TABLE) tally_pss_record<true, false, true>(P, LdsTableRowMajor{dyn_lds, rows}, NoSite{}, src, h, pl);
                else tally_pss_record<true, false, true>(P, GlobalTable{P.counters, P.off_rev}, NoSite{}, src, h, pl);
            } else if (P.off_site) {   // -X: the in-context pair takes its adds straight in the counter block
                const GlobalSite site{P.counters + P.off_site, rows * 16u};
                if (LDS_TABLE) tally_pss_record<true, true>(P, LdsTableRowMajor{dyn_lds, rows}, site, src, h, pl);
                else tally_pss_record<true, true>(P, GlobalTable{P.counters, P.off_rev}, site, src, h, pl);
            } else if (LDS_TABLE) tally_pss_record<true>(P, LdsTableRowMajor{dyn_lds, rows}, src, h, pl);
            else tally_pss_record<true>(P, GlobalTable{P.counters, P.off_rev}, src, h, pl);
            // -E: the conditional pair and reads[] take their adds straight in the counter block
            if (P.end_depth) tally_end_condition<true>(P, GlobalEndTable{P.counters + P.off_end, rows * 16u}, src, h, pl);
            // -H: straight into the counter block (hist_lds_bins is 0 in this kernel's launches)
            if (P.hist_max) hist_add(P, nullptr, hist_bin(P, pl.L), pl.pss_fwd, pl.pss_rev, 1u);
            // -N: likewise
            if (P.mism_hist) mism_add(P, nullptr, mism_bin(P, mm), pl.pss_fwd, pl.pss_rev, 1u);
            // -Y: likewise
            if (P.score_half) score_add(P, nullptr, score_bin(P, sc), pl.pss_fwd, pl.pss_rev, 1u);
            // -W: the read's interior, once, whichever table took the read
            if (P.interior) count_interior(P, src, h, P.genome + pl.gbase, pl.s, pl.L, pl.rev);
            // -P: the reference around the 5' end of a read in the forward table, around the 3' end of one in the reverse table
            if (P.composition) count_composition(P, P.genome + pl.gbase, contig_length(P, h), pl.s, pl.L, pl.rev, pl.pss_fwd, pl.pss_rev);
        }
        bool kfail = false;
        if (pl.fk5 || pl.fk3) kfail = tally_kmer_record<false>(P, pl, nullptr);
        book_events(do_pss, do_kmer, record_events(do_pss, do_kmer, pl, kfail), lds_delta);
    }
    __syncthreads();
    if (LDS_TABLE) {
        for (uint32_t i = threadIdx.x; i < tab_words; i += blockDim.x) {
            const uint32_t v = dyn_lds[i];
            if (v) {
                const uint32_t table = i / (rows * 16u), rest = i % (rows * 16u);
                atomicAdd(&P.counters[(table ? P.off_rev : 0u) + rest], (unsigned long long)v);
            }
        }
    }
    flush_events(do_pss, do_kmer, P, lds_delta);
}

// ---------------------------------------------------------------------------------------
// tally_tiled
// ---------------------------------------------------------------------------------------
// LDS objects.  Only the staging buffer is dynamic (extern) LDS; everything else is a
// separate static object:
//   stage  (dynamic) : T * P * 16 + STAGE_SLACK          first P pieces of every record of the tile
//   sheet  : TILED_MAX_T * 64                             code sheet [read][end*32 + position]
//   table  : 64 * 32 * 4                                  [(cell<<1)|table][row] u32; codes 32..63 = trash bin
//                                                         for "no count" codes, so the column pass has no branches
//   toffs  : 2 * (TILED_MAX_T + 4) * 4                    record offsets of this tile and the next
//   kmer   : 2 * 4^KMER_LDS_MAX_K * 4                     (LDS_KMER variants only)
//   refs   : (REF_LDS_ENTRIES + 1) * 16                   contig info of the first BAM references
__host__ __device__ inline uint32_t tiled_lds_bytes(uint32_t T, uint32_t pieces) { return T * pieces * 16u + STAGE_SLACK; }

// Four dwords at 4-byte alignment: gfx950 global loads only need dword alignment, so this
// compiles to ONE global_load_dwordx4 per lane.  A gather's cost in the texture addresser is per
// wave-instruction and per distinct line touched -- nine single-dword gathers of a 36-byte
// window cost three times what 2 x dwordx4 + 1 x dword do.
struct __attribute__((packed, aligned(4))) Quad { uint32_t v[4]; };
struct __attribute__((packed, aligned(4))) Tri { uint32_t v[3]; };

// -n / -N and -W, tiled form: the walk over read bases lo .. hi - 1 of a record whose SEQ starts at LDS byte seq_at of `stage`;
// g0 = the genome position of read base 0, lo a multiple of 8.  32 bases per round trip: five genome dwords gathered like an
// end window (one dwordx4 + one dword, brought to the read's alignment with v_alignbit) against 16 SEQ bytes, whose nibbles
// are swapped into the genome image's order (even position = low nibble).  The gather may run up to 39 positions past
// hi and the SEQ reads 19 bytes: inside the padding between contigs (CONTIG_PAD) and inside STAGE_SLACK; what they bring is masked.
// step(W, R, keep, p): eight positions from p on -- nibble q of W / R = the reference / read nibble of position p + q, keep =
// the nibbles of the positions below hi.
template <class Step>
__device__ __forceinline__ void walk_read_staged(const uint32_t *genome4, uint64_t g0, const uint8_t *stage, uint32_t seq_at,
                                                 uint32_t lo, uint32_t hi, Step step) {
    for (uint32_t b = lo; b < hi; b += 32u) {
        const uint64_t ga = g0 + b;
        const uint32_t *pg = genome4 + (ga >> 3);
        const Quad q = *(const Quad *)pg;
        const uint32_t gq[5] = {q.v[0], q.v[1], q.v[2], q.v[3], pg[4]};
        const uint32_t gsh = 4u * (uint32_t)(ga & 7ull);
        const uint32_t sa = seq_at + (b >> 1);
        const uint32_t *qs = (const uint32_t *)(stage + (sa & ~3u));
        uint32_t sr[5];
#pragma unroll
        for (int k = 0; k < 5; k++) sr[k] = qs[k];
        const uint32_t left = hi - b;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t have = left > 8u * t ? min(left - 8u * t, 8u) : 0u;
            const uint32_t W = __builtin_amdgcn_alignbit(gq[t + 1], gq[t], gsh);
            const uint32_t S = __builtin_amdgcn_alignbyte(sr[t + 1], sr[t], sa & 3u);
            const uint32_t R = ((S >> 4) & 0x0F0F0F0Fu) | ((S & 0x0F0F0F0Fu) << 4);
            const uint32_t keep = have >= 8u ? 0xFFFFFFFFu : (1u << (4u * have)) - 1u;
            step(W, R, keep, b + 8u * t);
        }
    }
}
// -n / -N: the mismatches among read bases lo .. hi - 1
__device__ __forceinline__ uint32_t count_mismatches_staged(const uint32_t *genome4, uint64_t g0, const uint8_t *stage, uint32_t seq_at,
                                                            uint32_t lo, uint32_t hi, bool tv_only) {
    uint32_t m = 0u;
    walk_read_staged(genome4, g0, stage, seq_at, lo, hi,
                     [&](uint32_t W, uint32_t R, uint32_t keep, uint32_t) { m += (uint32_t)__popc(mismatch_flags8(W, R, tv_only) & keep); });
    return m;
}

// -y / -Y: the score's share of read bases lo .. hi - 1 (read_score is the definition).  Eight positions a step: the nibbles where the
// reference is C and the read C or T, or the reference G and the read G or A, are found nibble-parallel (a BAM read nibble is
// one-hot: A 1, C 2, G 4, T 8); only those -- about half of a read -- fetch their QUAL byte from the staged record (qual_at: LDS byte
// of QUAL[0]) and their weight from the table in global memory.  A staged record has fewer than 2048 bases: 32 bits hold the sum.
template <bool MASKQ>
__device__ __forceinline__ int32_t read_score_staged(const TallyParams &P, uint64_t g0, const uint8_t *stage, uint32_t seq_at, uint32_t qual_at,
                                                     uint32_t lo, uint32_t hi, uint32_t L, bool rev) {
    int32_t S = 0;
    const uint32_t nd1 = P.score_nd - 1u, nq1 = P.score_nq - 1u;
    const int16_t *__restrict__ w = P.score_w;
    walk_read_staged(P.genome4, g0, stage, seq_at, lo, hi, [&](uint32_t W, uint32_t R, uint32_t keep, uint32_t p) {
        const uint32_t K = 0x11111111u;
        const uint32_t g_lo = W & K, g_hi = (W >> 1) & K, g_other = ((W >> 2) | (W >> 3)) & K;
        const uint32_t is_c = g_lo & ~g_hi & ~g_other, is_g = g_hi & ~g_lo & ~g_other;
        const uint32_t r_a = R & K, r_c = (R >> 1) & K, r_g = (R >> 2) & K, r_t = (R >> 3) & K;
        const uint32_t mis = (is_c & r_t & ~(r_a | r_c | r_g)) | (is_g & r_a & ~(r_c | r_g | r_t));   // C->T, G->A
        uint32_t m = (mis | (is_c & r_c & ~(r_a | r_g | r_t)) | (is_g & r_g & ~(r_a | r_c | r_t))) & keep;
        while (m) {
            const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            const uint32_t i = p + (bit >> 2);
            const uint32_t qv = stage[qual_at + i];
            if (MASKQ && qv < P.min_bq) continue;
            const bool at_c = (is_c >> bit) & 1u;
            const uint32_t kind = ((at_c != rev) ? 0u : 2u) + ((mis >> bit) & 1u);
            const uint32_t d = at_c ? i : L - 1u - i;
            S += w[(kind * P.score_nd + min(d, nd1)) * P.score_nq + min(qv, nq1)];
        }
    });
    return S;
}

constexpr uint32_t TILED_MAX_T = 128;
static_assert(TILED_MAX_T * 2 == TILED_THREADS, "CODES maps one (read, end) pair to each thread");

// STAGE: piece q of the tile (q = record * P + piece) goes to stage + q*16.  Each wave-instruction
// moves 64 consecutive pieces (1 KiB of LDS); a lane's source is its record's 16-byte aligned
// start + 16 * piece.  Pieces that would start beyond the record block are not issued.
//
// The LDS-DMA instruction is issued through inline asm on purpose.  hipcc's waitcnt pass
// fences EVERY later LDS access behind vmcnt(0) once it has seen an LDS-DMA it cannot
// disambiguate (no alias-scope metadata reaches it from HIP source), which would serialise
// the transfer against the passes it is meant to hide behind.  The asm form is invisible to
// that pass; ordering is ours: the kernel waits with an explicit `s_waitcnt vmcnt(0)` + barrier
// before any lane reads `stage`, and nothing else writes `stage`.  (Compiler-counted vmcnt(N)
// waits for its own loads only get stricter with unseen operations in flight, never weaker:
// vmcnt retires in order.)
//
// The pieces are loaded with the nontemporal policy (`nt`): the record stream is read exactly once
// per launch and is many times the L2 and MALL, so keeping its lines only evicts the reference
// windows, which neighbouring reads do re-read (those gathers keep the default policy).  The C3
// launch is bound by this stream -- switching the whole CODES phase off takes only 3 % off it
//  -- and `nt` lets it run closer to the chip's plain streaming rate.
__device__ __forceinline__ void stage_tile_dma(const uint8_t *recs, uint64_t recs_limit, const uint32_t *tile_offs,
                                               uint32_t count, uint32_t pieces, uint8_t *stage, uint32_t tid) {
    const uint32_t n_pieces = count * pieces;
    const uint32_t lds0 = (uint32_t)(uintptr_t)stage;  // LDS byte address (low half of the generic pointer)
    // q / pieces by multiply-shift: exact for q < 2^13 and pieces <= 64 ((pieces-1) * q < 2^20)
    const uint32_t magic = ((1u << 20) + pieces - 1u) / pieces;
    for (uint32_t q0 = (tid & ~63u); q0 < n_pieces; q0 += TILED_THREADS) {
        const uint32_t q = q0 + (tid & 63u);
        const uint32_t jq = (q * magic) >> 20;
        const uint32_t j = min(jq, count - 1u), pc = q - jq * pieces;
        const uint64_t a = (uint64_t)(tile_offs[j] & ~15u) + 16u * pc;
        if (q < n_pieces && a + 16u <= recs_limit) {
            const uint8_t *src = recs + a;
            const uint32_t m0v = __builtin_amdgcn_readfirstlane(lds0 + (q0 << 4));
            uint32_t keep;   // m0 is compiler-reserved and cannot be named as a clobber: save and restore it
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(m0v) : "memory");
        }
    }
}

// The arm of a tally_tiled launch: what it computes beside the tables, for one of the options that exclude each other
// (-H, -X, -E, -I, -n / -N, -W, -P, -y / -Y; engine.hip: MODES).  At most one, so it is one template argument.
enum TallyArm { ARM_NONE, ARM_HIST, ARM_SITE, ARM_END, ARM_GAPPED, ARM_MISM, ARM_INTERIOR, ARM_COMP, ARM_SCORE };

// Which tally_tiled<DO_PSS, DO_KMER, LDS_KMER, LATER, MASKQ, REGIONS, ARM> exist (REGIONS is free): the k-mer bins are in LDS only
// where there is a k-mer tally, base qualities mask the substitution tables only, a later pass (rows 32.. of a large -r) is
// the substitution tally alone; the length histogram belongs to pass 0 and may sit beside the k-mer tally, site context and
// anchored ends go with the substitution tally alone in every pass, every other arm with pass 0 of it.
constexpr bool tally_tiled_exists(bool DO_PSS, bool DO_KMER, bool LDS_KMER, bool LATER, bool MASKQ, TallyArm ARM) {
    const bool pss_alone = DO_PSS && !DO_KMER;
    return (DO_PSS || DO_KMER) && (DO_KMER || !LDS_KMER) && (DO_PSS || !MASKQ) && (!LATER || pss_alone) &&
           (ARM == ARM_NONE || (ARM == ARM_HIST ? DO_PSS && !LATER : ARM == ARM_SITE || ARM == ARM_GAPPED ? pss_alone : pss_alone && !LATER));
}

// A record too large for the staging window: decoded and tallied straight from global memory
// by one lane.  Rare (a record of tens of KB); kept out of line so it costs the hot path
// nothing.  It reads the kernel arguments through a pointer to the kernarg segment (taken in
// the kernel): a reference to the kernel's by-value copy would force that whole struct into
// scratch memory.
template <bool DO_PSS, bool DO_KMER, bool LDS_KMER, bool MASKQ = false, bool REGIONS = false, TallyArm ARM = ARM_NONE>
__device__ __attribute__((noinline)) uint32_t tally_overflow_record(const TallyParams *kernarg, uint32_t o0,
                                                                    uint32_t o1, uint32_t *table, uint32_t *lds_kmer,
                                                                    uint32_t *hist_lds = nullptr, uint32_t *site_lds = nullptr,
                                                                    uint32_t *end_lds = nullptr) {
    constexpr bool HIST = ARM == ARM_HIST, SITE = ARM == ARM_SITE, END = ARM == ARM_END, GAPPED = ARM == ARM_GAPPED, MISM = ARM == ARM_MISM,
                   INTERIOR = ARM == ARM_INTERIOR, COMP = ARM == ARM_COMP, SCORE = ARM == ARM_SCORE;
    const TallyParams &P = *kernarg;
    GlobalBytes gsrc{P.recs + o0};
    const RecHdr gh = decode_hdr(gsrc, o1 - o0);
    auto gpl = make_plan<DO_PSS, DO_KMER, REGIONS, GAPPED>(P, gsrc, gh);   // (GAPPED: walks every CIGAR op)
    [[maybe_unused]] uint32_t mm = 0u;
    if constexpr (MISM) {   // (hist_lds: the MISM instantiation's LDS bins)
        if (gpl.pss_fwd || gpl.pss_rev) {
            mm = count_mismatches(gsrc, gh, P.genome + gpl.gbase, gpl.s, gpl.L, P.mism_tv != 0u);
            if (mism_beyond(P, mm)) gpl.pss_fwd = gpl.pss_rev = false;
            else if (P.mism_hist) mism_add(P, hist_lds, mism_bin(P, mm), gpl.pss_fwd, gpl.pss_rev, 1u);
        }
    }
    if constexpr (SCORE) {   // (hist_lds: the SCORE instantiation's LDS bins)
        if (gpl.pss_fwd || gpl.pss_rev) {
            const int32_t sc = read_score(P, gsrc, gh, P.genome + gpl.gbase, gpl.s, gpl.L, gpl.rev);
            if (score_below(P, sc)) gpl.pss_fwd = gpl.pss_rev = false;
            else if (P.score_half) score_add(P, hist_lds, score_bin(P, sc), gpl.pss_fwd, gpl.pss_rev, 1u);
        }
    }
    if constexpr (GAPPED) {
        if (gpl.pss_fwd || gpl.pss_rev) tally_pss_record<MASKQ, false, true>(P, LdsTableColumnMajor{table, P.row_base}, NoSite{}, gsrc, gh, gpl);
    } else if constexpr (SITE) {
        if (gpl.pss_fwd || gpl.pss_rev)
            tally_pss_record<MASKQ, true>(P, LdsTableColumnMajor{table, P.row_base}, LdsSiteColumnMajor{site_lds, P.row_base}, gsrc, gh, gpl);
    } else if (DO_PSS && (gpl.pss_fwd || gpl.pss_rev)) tally_pss_record<MASKQ>(P, LdsTableColumnMajor{table, P.row_base}, gsrc, gh, gpl);
    if constexpr (HIST) {   // (the HIST instantiation is a pass-0 one: counted once)
        if (gpl.pss_fwd || gpl.pss_rev) hist_add(P, hist_lds, hist_bin(P, gpl.L), gpl.pss_fwd, gpl.pss_rev, 1u);
    }
    if constexpr (END) tally_end_condition<MASKQ>(P, LdsEndTable{end_lds, (uint32_t)P.N + 2u}, gsrc, gh, gpl);   // (a pass-0 one as well)
    if constexpr (INTERIOR) {   // (likewise; straight into the counter block)
        if (gpl.pss_fwd || gpl.pss_rev) count_interior(P, gsrc, gh, P.genome + gpl.gbase, gpl.s, gpl.L, gpl.rev);
    }
    if constexpr (COMP) {   // (likewise)
        if (gpl.pss_fwd || gpl.pss_rev) count_composition(P, P.genome + gpl.gbase, contig_length(P, gh), gpl.s, gpl.L, gpl.rev, gpl.pss_fwd, gpl.pss_rev);
    }
    bool kfail = false;
    if (DO_KMER && (gpl.fk5 || gpl.fk3)) kfail = tally_kmer_record<LDS_KMER>(P, gpl, lds_kmer);
    return record_events(DO_PSS, DO_KMER, gpl, kfail);
}

// What picks a read's table plane in tally_tiled_body: nothing (one plane), its first RG:Z value
// (-G), its length bin (-S), its contig's set (-C), its refID itself (-A: a plane per BAM reference), or a hash of its
// read name (-J: the jackknife replicates).
enum PlaneSel { PLANES_NONE = 0, PLANES_RG, PLANES_LEN, PLANES_REF, PLANES_EACH, PLANES_HASH };

// ---- -A: a plane per reference ---------------------------------------------------------------------------------
// Plane k is refID k, plane n_ref (= n_groups - 1) the refID -1 records; only a record whose reference was found is ever
// added to a table, so any other refID never asks.  Unlike the planes of -G / -S / -C these are not a fixed short list
// of a launch: a workgroup keeps the planes of the few references its tiles meet in LDS slots (each_lds below) and adds
// them to the counter block itself.
constexpr uint32_t EACH_MAX_SLOTS = 32;       // LDS planes a workgroup can hold ($PSSBAM_CONTIG_SLOTS up to here)
constexpr uint32_t EACH_DEFAULT_SLOTS = 7;    // 7 + the trash plane = 32 KiB, what a one-pass -G / -S / -C launch takes at most
constexpr uint32_t EACH_EMPTY = 0xFFFFFFFFu;  // held[s]: no reference owns slot s
// each_lds: [held EACH_MAX_SLOTS | miss count | miss queue TILED_MAX_T | used EACH_MAX_SLOTS: 1 + the last tile iteration that met the slot]
constexpr uint32_t EACH_MISS_N = EACH_MAX_SLOTS, EACH_MISSQ = EACH_MAX_SLOTS + 1u, EACH_USED = EACH_MISSQ + 128u, EACH_LDS_WORDS = EACH_USED + EACH_MAX_SLOTS;
__device__ __forceinline__ uint32_t each_plane(const RecHdr &h, const PlaneParams &G) { return min((uint32_t)h.ref_id, G.n_groups - 1u); }
__device__ __forceinline__ uint64_t each_plane_base(const PlaneParams &G, uint32_t plane) {
    return (uint64_t)G.off_groups + (uint64_t)plane * G.plane_words;
}
__device__ __forceinline__ uint64_t each_touched_base(const PlaneParams &G) { return each_plane_base(G, G.n_groups); }   // one word per plane
struct GlobalPlaneTable {  // rows row_base .. row_base + n_rows - 1 straight into one plane of the counter block
    unsigned long long *c;
    uint32_t *hit;          // set when something was added: the caller then stores the plane's touched word, once per record
    uint32_t off_rev, row_base, n_rows;
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        if (row - row_base < n_rows) {
            atomicAdd(&c[(table ? off_rev : 0u) + row * 16u + cell], 1ull);
            *hit = 1u;
        }
    }
};

// KMER: the plane of the k-mer tally -- its length bins go by Plan::Lk (strlen(SEQ), what fragkon's -l / -L compare,
// for paired reads too), not by Plan::L.
template <PlaneSel PLANES, bool KMER = false, class Src>
__device__ __forceinline__ uint32_t record_plane(const Src &src, const RecHdr &h, const Plan &pl, const PlaneParams &G) {
    if constexpr (PLANES == PLANES_RG) return read_group_plane(src, h, G);
    else if constexpr (PLANES == PLANES_EACH) return each_plane(h, G);
    else if constexpr (PLANES == PLANES_REF) return pl.ref_plane;   // from the ref_info entry plan_head loaded
    else if constexpr (PLANES == PLANES_HASH) return 1u + read_name_replicate(src, h.rec_len, G.n_groups);   // K = n_groups
    else return length_bin_plane(G, KMER ? pl.Lk : pl.L);
}

// ---- k-mer planes --------------------------------------------------------------------------------------------
// First word of plane `plane`'s [k5 | k3] pair in the counter block.  64-bit: a plane is 2 * 4^k words.
__device__ __forceinline__ uint64_t kmer_plane_base(const TallyParams &P, const PlaneParams &G, uint32_t plane) {
    return plane ? G.koff_planes + (uint64_t)(plane - 1u) * G.kplane_words : (uint64_t)P.off_k5;
}
// One bin of table `which` (0 = 5', 1 = 3') of plane `plane`: into the plane's slot of the launch's LDS histograms
// (a plane outside plane0 .. plane0 + n_slots - 1 lands in the trash slot behind them), or straight into the
// counter block.
template <bool LDS_KMER>
__device__ __forceinline__ void kmer_plane_add(const TallyParams &P, const PlaneParams &G, uint32_t plane, uint32_t which,
                                               uint32_t bin, uint32_t *lds_kmer) {
    const uint32_t nb = 1u << (2 * P.K);
    if (LDS_KMER) {
        const uint32_t slot = min(plane - G.plane0, G.n_slots);   // (plane < plane0 wraps: trash as well)
        atomicAdd(&lds_kmer[slot * 2u * nb + (which ? nb : 0u) + bin], 1u);
    } else {
        atomicAdd(&P.counters[kmer_plane_base(P, G, plane) + (which ? nb : 0u) + bin], 1ull);
    }
}
// tally_kmer_record for a record of plane `plane` (lane-per-read form); true = an attempted add failed
template <bool LDS_KMER>
__device__ __forceinline__ bool tally_kmer_record_plane(const TallyParams &P, const PlaneParams &G, const Plan &pl, uint32_t plane,
                                                        uint32_t *lds_kmer) {
    const uint8_t *Gn = P.genome + pl.gbase;
    int64_t w5, w3;
    kmer_windows(pl, P.K, w5, w3);
    bool good = true;
    for (uint32_t which = 0; which < 2u; which++) {   // both attempted, independently (fragkon.c:164-181)
        if (!(which ? pl.fk3 : pl.fk5)) continue;
        uint32_t bin;
        if (kmer_bin(Gn, which ? w3 : w5, P.K, pl.rev, bin)) kmer_plane_add<LDS_KMER>(P, G, plane, which, bin, lds_kmer);
        else good = false;
    }
    return !good;
}
// tally_overflow_record for tally_tiled_kmer_planes
template <PlaneSel PLANES, bool LDS_KMER, bool REGIONS = false>
__device__ __attribute__((noinline)) uint32_t tally_overflow_record_kmer_planes(const TallyParams *kernarg, const PlaneParams *gk,
                                                                                uint32_t o0, uint32_t o1, uint32_t *lds_kmer) {
    const TallyParams &P = *kernarg;
    GlobalBytes gsrc{P.recs + o0};
    const RecHdr gh = decode_hdr(gsrc, o1 - o0);
    const Plan gpl = make_plan<false, true, REGIONS>(P, gsrc, gh);
    bool kfail = false;
    if (gpl.fk5 || gpl.fk3) kfail = tally_kmer_record_plane<LDS_KMER>(P, *gk, gpl, record_plane<PLANES, true>(gsrc, gh, gpl, *gk), lds_kmer);
    return record_events(false, true, gpl, kfail);
}

// The same for tally_tiled_planes (substitution tables only): the record's plane slot of this
// launch, if it has one, decides where its counts go.  (PLANES_EACH: also the path of a read that found no free slot.)
template <PlaneSel PLANES, bool MASKQ = false, bool REGIONS = false>
__device__ __attribute__((noinline)) uint32_t tally_overflow_record_planes(const TallyParams *kernarg, const PlaneParams *gk,
                                                                           uint32_t o0, uint32_t o1, uint32_t *table) {
    const TallyParams &P = *kernarg;
    GlobalBytes gsrc{P.recs + o0};
    const RecHdr gh = decode_hdr(gsrc, o1 - o0);
    const Plan gpl = make_plan<true, false, REGIONS>(P, gsrc, gh);
    if constexpr (PLANES == PLANES_EACH) {   // -A: no slot is needed, the rows of this pass go straight into the reference's plane
        if (gpl.pss_fwd || gpl.pss_rev) {
            const uint32_t plane = each_plane(gh, *gk);
            uint32_t hit = 0u;
            tally_pss_record<MASKQ>(P, GlobalPlaneTable{P.counters + each_plane_base(*gk, plane), &hit, P.off_rev, P.row_base, 32u}, gsrc, gh, gpl);
            if (hit) P.counters[each_touched_base(*gk) + plane] = 1ull;
        }
    } else
    if (gpl.pss_fwd || gpl.pss_rev) {
        const uint32_t slot = record_plane<PLANES>(gsrc, gh, gpl, *gk) - gk->plane0;
        if (slot < gk->n_slots) tally_pss_record<MASKQ>(P, LdsTableColumnMajor{table + slot * GROUP_PLANE_WORDS, P.row_base}, gsrc, gh, gpl);
    }
    return record_events(true, false, gpl, false);
}

// -Q: byte mask of one dword of QUAL bytes: 0xFF where the byte is below q (q4 = q in every byte, 1 <= q <= 93), else
// 0x00.  (x | 0x80) - q cannot borrow from the next byte (q < 0x80) and leaves bit 7 clear exactly when
// (x & 0x7F) < q; bytes >= 0x80 (the 0xFF fill of absent qualities) are taken out by ~x.
__device__ __forceinline__ uint32_t base_quality_mask(uint32_t x, uint32_t q4) {
    const uint32_t lt = ~((x | 0x80808080u) - q4) & ~x & 0x80808080u;
    return (lt - (lt >> 7)) | lt;   // 0x80 -> 0xFF
}

// -W, tiled form: read bases lo .. hi - 1 of a staged record (walk_read_staged; lo a multiple of 8) into this lane's 16 bins,
// of which only the positions from d on count -- the interior has a low edge as well as a high one.  MASKQ: the same eight
// positions' QUAL bytes come out of `stage` too (a whole record is staged under -Q; three aligned dwords at qual_at + p, at most
// 11 bytes past QUAL, inside the record's aux fields, the next record or STAGE_SLACK), base_quality_mask's 0xFF bytes become the
// nibbles of `keep`.  The counts leave as 16-bit pairs, pk[k] = bins 2k | 2k + 1 << 16: a staged record is at most 64 pieces
// of 16 bytes, fewer than 2048 bases.
template <bool MASKQ>
__device__ __forceinline__ void count_interior_staged(const uint32_t *genome4, uint64_t g0, const uint8_t *stage, uint32_t seq_at, uint32_t qual_at,
                                                      uint32_t lo, uint32_t hi, uint32_t d, uint32_t min_bq, uint32_t (&pk)[8]) {
    uint32_t cnt[16];
#pragma unroll
    for (int k = 0; k < 16; k++) cnt[k] = 0u;
    walk_read_staged(genome4, g0, stage, seq_at, lo, hi, [&](uint32_t W, uint32_t R, uint32_t keep, uint32_t p) {
        if (p < d) keep &= d - p >= 8u ? 0u : ~((1u << (4u * (d - p))) - 1u);
        if constexpr (MASKQ) {
            const uint32_t qa = qual_at + min(p, hi);   // (a step wholly past hi keeps nothing: it stays where the last one read)
            const uint32_t *qp = (const uint32_t *)(stage + (qa & ~3u));
            const uint32_t q4 = min_bq * 0x01010101u;
            uint32_t low = 0u;
#pragma unroll
            for (int w = 0; w < 2; w++) {   // byte i of dword w = QUAL[p + 4w + i] -> nibble 4w + i
                const uint32_t x = base_quality_mask(__builtin_amdgcn_alignbyte(qp[w + 1], qp[w], qa & 3u), q4);
                low |= ((x & 0xFu) | ((x >> 4) & 0xF0u) | ((x >> 8) & 0xF00u) | ((x >> 12) & 0xF000u)) << (16 * w);
            }
            keep &= ~low;
        }
        interior_step8(W, R, keep, cnt);
    });
#pragma unroll
    for (int k = 0; k < 8; k++) pk[k] = cnt[2 * k] | (cnt[2 * k + 1] << 16);
}

// Reference windows, one per alignment end, each with STATIC byte positions:
//   left  end (e = 0): 32 bytes from s-2      byte w <-> row w          (0,1 context; 2+i = position i)
//   right end (e = 1): 32 bytes up to s+L+1   byte w <-> row 31-w       (31 -> row 0, 30 -> row 1, 29-i -> 2+i)
// Read bases: left row 2+i <-> base i ; right row 2+i <-> base L-1-i, i.e. window byte w <-> base (L-30)+w.
// The kernel body takes its LDS regions as __restrict__ pointers: after inlining, every LDS
// access carries alias-scope metadata, which is what lets the compiler see that the code sheet,
// the count table and the offset buffer never alias the LDS-DMA destination (`stage`) -- without
// it every LDS access issued while a DMA transfer is in flight is fenced behind vmcnt(0) and
// the transfer cannot overlap the COLUMNS pass.
//
// PLANES_RG / PLANES_LEN (-G / -S, tally_tiled_planes): `table` holds gk->n_slots
// planes of [(cell<<1)|table][row] plus one trash plane behind them; every read's plane slot is
// resolved in CODES-A (record_plane: read_group_plane or length_bin_plane) and kept in grp_lds, and
// COLUMNS adds the wave's scalar slot offset to each real code.
//
// PLANES_HASH (-J, tally_tiled_planes): the same path; the left-end lane of every candidate hashes the read name from the
// staged bytes in CODES-A (read_name_replicate: the name lies in front of SEQ, so a staged prefix holds it), in front of
// the barrier that releases `stage`, one loop iteration per four name bytes.  Prefixes are staged as without it, and
// COLUMNS does not change.  A record that is not staged takes the one-lane path, which hashes from global memory.
//
// PLANES_EACH (-A, tally_tiled_planes): a plane per BAM reference, far more than LDS holds, of which one tile touches a
// handful.  `table` holds gk->n_slots resident planes plus the trash plane, `each_lds` the refIDs that own them
// (held[], EACH_EMPTY = free).  In CODES-A the left-end lane of every candidate finds its reference's slot in held[] or
// claims the first free one with an LDS compare-and-swap -- all lanes scan in slot order and a slot never changes
// owner during the phase, so the lanes of one reference agree -- and COLUMNS runs as for the other selectors.  Slots
// live across the tiles a workgroup walks.  A read that finds every slot taken does not wait: its codes go to the
// trash plane, it is queued, and behind COLUMNS one lane tallies it straight into its plane of the counter block
// (tally_overflow_record_planes, 64-bit atomics).  A tile that had such a miss ends by flushing and emptying every
// slot, and so does a tile that leaves every slot taken without having used them all (gk->each_evict != 0; it is 0 only for
// A/B runs): on a coordinate-sorted input a workgroup meets one reference after the other, and emptying the full table
// behind the tile keeps the next reference from finding no slot -- which would send a whole tile of reads down the
// one-lane path; a tile that uses every slot gains nothing from it and is left alone.  The kernel ends with the same
// flush: every non-zero word of a held plane is added to the counter block with
// one 64-bit atomic, the plane's touched flag is set and the LDS word zeroed.  The planes take no scratch slot and no
// reduce; the status deltas keep theirs.  The other instantiations contain none of it.
//
// MASKQ (-Q, min_bq > 0): whole records are staged (QUAL lies behind SEQ), CODES-A also fetches the 32 QUAL bytes
// that line up with the end's window and CODES-B turns them into a 0x00 / 0xFF byte per position that is ORed into
// the read-side code: a position whose base quality is below P.min_bq lands on a trash code, exactly like a read
// base that is not A/C/G/T.  The instantiations without MASKQ contain none of it.
//
// REGIONS (-T, P.region_info != NULL): every candidate's alignment is looked up in the region table in CODES-A.  The
// contig's descriptor is fetched right behind plan_head, the two grid words behind the window gathers -- so the round
// trips overlap -- and the interval compare is resolved where the gathered registers are first used, in front of the
// next tile's DMA: a candidate that meets no region stops being one before -U/-D is decided and before the k-mer add.
// Both lanes of a read's pair ask (same addresses: one request to the memory system).  Only the record's fixed fields
// are read, so prefixes are staged as without it.  The instantiations without REGIONS contain none of it.
//
// The arms (ARM: one per instantiation at the most, and which instantiations exist says tally_tiled_exists):
//
// HIST (-H, P.hist_max > 0; pass 0, one plane): behind CODES-B, where pss_fwd / pss_rev are decided, the left-end lane
// of every read that is added to a table counts its length (hist_wave_add); `hist_lds` holds the LDS part of the two
// arrays and is added to the counter block when the workgroup is done, one 64-bit atomic per non-zero bin.  Nothing is
// read that the kernel does not read anyway.  The instantiations without HIST contain none of it.
//
// SITE (-X cpg, P.off_site != 0; one plane, substitution tables only): CODES-B compares the window's reference codes with
// their one-base neighbours -- GE / GO against each other shifted by a byte -- and sets CODE_SITE in the sheet byte of
// every interior position whose reference position is in CpG context; COLUMNS adds such a position a second time, into
// the 2 KiB in-context table `site_lds` (SITE_WORDS).  The neighbour beyond either edge of the window (one nibble each)
// comes with the window gather in CODES-A: the one behind it lies in the fifth gathered dword already, the one in
// front of it is one more dword load of a line the gather touches anyway.  The instantiations without SITE contain
// none of it.
//
// END (-E, P.end_depth > 0; pass 0 of a one-pass launch, one plane, substitution tables only): when CODES-B has formed a
// lane's codes -- table coordinates, -Q and the blanking of absent bases applied -- the lane compares rows 2 .. 2 + depth - 1
// of its own end with the wanted code ((cell5 << 1) on the lane that feeds the forward table, (cell3 << 1) | 1 on the one that
// feeds the reverse table), all of them at once on the four code words that hold them.  The two lanes of a read's pair
// exchange the result, and a lane whose PARTNER is marked sets CODE_END in all its sheet bytes: COLUMNS adds a real code
// that carries it a second time, into the conditional tables `end_lds` behind the staging buffer ((N + 2) rows per code,
// end_lds_bytes).  The left-end lanes count reads[4] with a ballot each.  The instantiations without END contain none of it.
//
// GAPPED (-I, P.gapped; one plane, substitution tables only, every pass): plan_head walks the CIGAR in the staged prefix (it lies in
// front of SEQ; at most GAPPED_TILED_OPS ops, a record with more takes the one-lane path) and returns the read-side anchors.  The
// reference side -- window, context bases, bounds, -T's interval [s, s + L) -- stays as it is; the read stream (and -Q's QUAL
// stream) of a left lane starts at q0 - 2, that of a right lane ends at q1, and CODES-B blanks a lane's positions outside
// [q0, q0 + a) / [q1 - b, q1) with the byte masks of the l_seq blanking, skipped wave-wide when no lane needs it.  The
// instantiations without GAPPED contain none of it.
//
// MISM (-n / -N / -V, P.mism_limit or P.mism_hist non-zero; pass 0 of a one-pass launch, one plane, substitution tables only): in
// CODES-A every lane of a candidate's pair compares one half of the read with the reference (count_mismatches_staged; the
// halves are cut at a multiple of 8 bases so that both start on a whole SEQ byte) and the two lanes add their counts with
// the exchange END uses.  All of it sits in front of the barrier that releases `stage`, so it reads the staged SEQ and
// has used its gathered genome dwords before the next tile's DMA is issued.  A read with m >= mism_limit stops being a
// candidate there, before -U/-D decide pss_fwd / pss_rev: its codes are "no count" and record_events books it as
// filtered.  Behind CODES-B the left-end lane of every read that is added to a table counts bin min(m, M + 1)
// (mism_wave_add) into `hist_lds`, here the 2 * (M + 2) words [mf | mr] behind the staging buffer, which leave LDS once, at
// kernel end, with one 64-bit atomic per non-zero bin.  The instantiations without MISM contain none of it.
//
// INTERIOR (-W, P.interior = d + 1 non-zero; pass 0 of a one-pass launch, one plane, substitution tables only): in
// CODES-A, where MISM compares, every lane of a candidate's pair walks one half of the read's interior [d, min(L - d, l_seq)) --
// the halves start at a multiple of 8 bases, d & ~7 and the cut, and the positions below d are masked -- and counts it into 16
// bins (count_interior_staged; under MASKQ with the staged QUAL bytes of the same positions).  Whether the read is added to a
// table is only known behind CODES-B (-U / -D need the window), so the counts cross the barrier as 16-bit pairs in eight
// VGPRs; there the lanes of the reads that were added merge per wave and add into the 17 words [table | reads] in `hist_lds`
// behind the staging buffer (interior_wave_add), the left-end lane counting the read.  The words leave LDS with one 64-bit
// atomic per non-zero word at kernel end, and every 8192 tiles of a workgroup: a tile adds fewer than 128 * 2048 = 2^18 to a
// word, so a u32 word cannot wrap.  The instantiations without INTERIOR contain none of it.
//
// COMP (-P, P.composition = w non-zero; pass 0 of a one-pass launch, one plane, substitution tables only):
// CODES-A gathers, next to the end's window, the 32 reference positions outside the read at this end (s - 32 .. s - 1 on the left,
// s + L .. s + L + 31 on the right: inside the padding between contigs where they leave the contig) and works out how many of the w
// outside offsets lie inside the contig; both are first used where the window's registers are, in front of the next tile's DMA.
// In CODES-B, once -U / -D have decided pss_fwd / pss_rev and in front of the forming of the code words, a lane whose end feeds
// a table lays the 64 nibbles around its end out in the order of the offsets -- a right end turned round -- and the wave adds
// them to the 20 w words [c5 | c3] in `hist_lds` behind the staging buffer (composition_wave_add): class by class, masked by
// position, a reverse-strand lane complemented.  The words leave LDS with one 64-bit atomic per non-zero word at kernel end,
// and every 8192 tiles of a workgroup: a tile adds at most 128 to a word, so a u32 word cannot wrap.  The instantiations
// without COMP contain none of it.
//
// SCORE (-y / -Y, P.score_w non-null; pass 0 of a one-pass launch, one plane, substitution tables only):
// in CODES-A, where MISM compares, every lane of a candidate's pair sums the weights of one half of [0, min(L, l_seq)), cut at a
// multiple of 8 bases (read_score_staged: SEQ and QUAL from the staged record -- a whole record is staged, as under -Q -- the
// reference from the 4-bit genome image, the weights from their table in global memory, which every workgroup re-reads and which
// therefore stays in L2), and the two lanes add their halves with the exchange MISM uses, in front of the barrier that releases
// `stage`.  With the filter a read below P.score_min stops being a candidate there, before -U/-D decide.  Behind CODES-B the
// left-end lane of every read that is added to a table counts its bin (bin_wave_add) into `hist_lds`, here the 4 * P.score_half
// words [sf | sr] behind the staging buffer, which leave LDS once, at kernel end, with one 64-bit atomic per non-zero word.  The
// instantiations without SCORE contain none of it.
template <bool DO_PSS, bool DO_KMER, bool LDS_KMER, bool LATER_PASS, PlaneSel PLANES = PLANES_NONE, bool MASKQ = false,
          bool REGIONS = false, TallyArm ARM = ARM_NONE>
__device__ __forceinline__ void tally_tiled_body(const TallyParams &P, const TallyParams *kernarg,
                                                 uint8_t *__restrict__ stage, uint8_t *__restrict__ sheet,
                                                 uint32_t *__restrict__ table,
                                                 uint32_t *__restrict__ toffs,
                                                 uint32_t *__restrict__ lds_kmer,
                                                 int32_t *__restrict__ lds_delta, uint4 *__restrict__ refs_lds,
                                                 const PlaneParams *gk = nullptr, uint32_t *__restrict__ grp_lds = nullptr,
                                                 uint32_t *__restrict__ hist_lds = nullptr, uint32_t *__restrict__ site_lds = nullptr,
                                                 uint32_t *__restrict__ end_lds = nullptr, uint32_t *__restrict__ each_lds = nullptr) {
    constexpr bool HIST = ARM == ARM_HIST, SITE = ARM == ARM_SITE, END = ARM == ARM_END, GAPPED = ARM == ARM_GAPPED, MISM = ARM == ARM_MISM,
                   INTERIOR = ARM == ARM_INTERIOR, COMP = ARM == ARM_COMP, SCORE = ARM == ARM_SCORE;
    constexpr bool GROUPED = PLANES != PLANES_NONE;   // one table plane per read group / length bin
    constexpr bool EACH = PLANES == PLANES_EACH;      // ... per BAM reference, resident in LDS slots
    static_assert(!EACH || (DO_PSS && !DO_KMER), "a plane per reference splits the substitution tables");
    constexpr bool KPLANES = GROUPED && DO_KMER;      // ... of k-mer bins (tally_tiled_kmer_planes: no sheet, no table)
    static_assert(!KPLANES || !DO_PSS, "planes split either the substitution tables or the k-mer tables");
    static_assert(tally_tiled_exists(DO_PSS, DO_KMER, LDS_KMER, LATER_PASS, MASKQ, ARM), "no such tally (tally_tiled_exists)");
    static_assert(ARM == ARM_NONE || PLANES == PLANES_NONE, "an arm belongs to the one-plane tally");
    const uint32_t T = P.reads_per_tile;   // <= TILED_MAX_T
    const uint32_t n_recs = P.n_recs_dev ? *P.n_recs_dev : P.n_recs;   // device-indexed blocks: the count lives in device memory
    const uint32_t pieces = P.prefix_pieces;  // 16-byte pieces staged per record
    const uint64_t recs_limit = (P.recs_bytes + 15ull) & ~15ull;  // the block is readable up to here
    const uint32_t ablate = P.ablate;      // diagnostics only (PSSBAM_ABLATE): 1 no COLUMNS, 2 no position loop, 4 no CODES, 128 no window gathers

    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const int N = P.N;
    const uint32_t n_pos = (uint32_t)N + 2u;  // rows per table: 2 context + N positions
    // this launch tallies rows row_base .. row_base+31 (window positions shifted accordingly);
    // pass 0 also owns the status counters and the k-mer tally
    // (a compile-time 0 in the first-pass instantiation: the common N <= 30 case pays nothing)
    const uint32_t row_base = LATER_PASS ? P.row_base : 0u;
    const bool pass0 = !LATER_PASS;
    const uint32_t n_live = n_pos > row_base ? min(n_pos - row_base, 32u) : 0u;

    // ---- one-time set-up: zero the tables ---------------------------------------------------------
    const uint32_t table_words = KPLANES ? 0u : GROUPED ? (gk->n_slots + 1u) * GROUP_PLANE_WORDS : TABLE_WORDS;
    for (uint32_t i = tid; i < table_words; i += TILED_THREADS) table[i] = 0u;
    uint32_t kmer_words = 2u * (1u << (2 * P.K));
    if constexpr (KPLANES) kmer_words *= gk->n_slots + 1u;   // one histogram per plane slot + the trash slot
    if (LDS_KMER)
        for (uint32_t i = tid; i < kmer_words; i += TILED_THREADS) lds_kmer[i] = 0u;
    if (tid < ST_USED) lds_delta[tid] = 0;
    if constexpr (HIST)
        for (uint32_t i = tid; i < 2u * P.hist_lds_bins; i += TILED_THREADS) hist_lds[i] = 0u;
    if constexpr (MISM)
        for (uint32_t i = tid; i < (P.mism_hist ? 2u * (P.mism_hist + 2u) : 0u); i += TILED_THREADS) hist_lds[i] = 0u;
    if constexpr (SCORE)
        for (uint32_t i = tid; i < 4u * P.score_half; i += TILED_THREADS) hist_lds[i] = 0u;
    if constexpr (INTERIOR)
        if (tid < INTERIOR_WORDS) hist_lds[tid] = 0u;
    // -W: the 17 LDS words into the counter block; an exchange, so that waves that are still adding lose nothing
    auto flush_interior = [&]() {
        if constexpr (INTERIOR) {
            if (tid < INTERIOR_WORDS) {
                const uint32_t v = atomicExch(&hist_lds[tid], 0u);
                if (v) atomicAdd(&P.counters[P.off_interior + tid], (unsigned long long)v);
            }
        }
    };
    [[maybe_unused]] const uint32_t comp_words = COMP ? 20u * P.composition : 0u;   // -P: [c5 | c3]
    if constexpr (COMP)
        for (uint32_t i = tid; i < comp_words; i += TILED_THREADS) hist_lds[i] = 0u;
    // -P: the LDS words into the counter block; an exchange, so that waves that are still adding lose nothing
    auto flush_composition = [&]() {
        if constexpr (COMP) {
            for (uint32_t i = tid; i < comp_words; i += TILED_THREADS) {
                const uint32_t v = atomicExch(&hist_lds[i], 0u);
                if (v) atomicAdd(&P.counters[P.off_composition + i], (unsigned long long)v);
            }
        }
    };
    if constexpr (SITE)
        for (uint32_t i = tid; i < SITE_WORDS; i += TILED_THREADS) site_lds[i] = 0u;
    if constexpr (END)
        for (uint32_t i = tid; i < 32u * n_pos + 4u; i += TILED_THREADS) end_lds[i] = 0u;
    if constexpr (EACH) {
        if (tid < EACH_MAX_SLOTS) { each_lds[tid] = EACH_EMPTY; each_lds[EACH_USED + tid] = 0u; }
        if (tid == 0u) each_lds[EACH_MISS_N] = 0u;
    }
    // -A: every held plane into the counter block, LDS words zeroed (the caller has put a barrier behind the last COLUMNS
    // pass and puts one in front of the next change of held[])
    auto flush_slots = [&]() {
        if constexpr (EACH) {
            // (every wave walks 64 consecutive words of ONE slot per round, all its lanes for the same number of rounds)
            for (uint32_t i = tid; i < gk->n_slots * GROUP_PLANE_WORDS; i += TILED_THREADS) {
                const uint32_t r = i & 31u;
                const uint32_t v = r < n_live ? table[i] : 0u;
                const unsigned long long any = __ballot(v != 0u);
                if (!any) continue;
                const uint32_t ref = each_lds[i / GROUP_PLANE_WORDS], ct = (i / 32u) & 31u;   // (a slot nobody owns holds zeros)
                if (v) {
                    atomicAdd(&P.counters[each_plane_base(*gk, ref) + ((ct & 1u) ? P.off_rev : 0u) + (row_base + r) * 16u + (ct >> 1)],
                              (unsigned long long)v);
                    table[i] = 0u;
                }
                if (lane == (uint32_t)__ffsll((long long)any) - 1u) P.counters[each_touched_base(*gk) + ref] = 1ull;   // once per wave and round
            }
        }
    };
    // contig info of the first BAM references (all of them for a human-sized header) + the "*" entry
    const uint32_t n_ref_cached = min((uint32_t)P.n_ref, REF_LDS_ENTRIES);
    if (tid < n_ref_cached) refs_lds[tid] = P.ref_info[tid];
    if (tid == n_ref_cached) refs_lds[tid] = P.ref_info[P.n_ref];
    const uint32_t all_tiles = (n_recs + T - 1u) / T;
    // Workgroup -> tiles.  Workgroups are dealt to the 8 XCDs round-robin (blockIdx & 7); with
    // xcd_map every XCD walks its own contiguous eighth of the block, so neighbouring tiles -- which
    // share reference lines and the record line at their seam -- meet in the same L2.
    uint32_t tile0 = blockIdx.x, tstride = gridDim.x, n_tiles = all_tiles;
    if (P.xcd_map && (gridDim.x & 7u) == 0u && all_tiles >= 64u) {
        const uint32_t per = (all_tiles + 7u) >> 3, xcd = blockIdx.x & 7u;
        tile0 = xcd * per + (blockIdx.x >> 3);
        tstride = gridDim.x >> 3;
        n_tiles = min(all_tiles, (xcd + 1u) * per);
    }
    // software pipeline over this workgroup's tiles k0, k0+stride, ...:
    //   toffs[par]      offsets of the tile being processed, toffs[par^1] those of the next one
    //                   (written from VGPRs that were loaded one tile earlier)
    //   stage           pieces of the tile being processed; refilled for the next tile as soon as
    //                   CODES-A has read everything it needs
    uint32_t tile = tile0;
    uint32_t off_a = 0;
    const uint32_t TOFF = TILED_MAX_T + 4u;  // stride between the two offset buffers
    auto load_offsets = [&](uint32_t t) {
        const uint32_t r0 = t * T;
        if (tid <= T && r0 + tid <= n_recs) off_a = P.offs[r0 + tid];
    };
    auto tile_count = [&](uint32_t t) { return min(T, n_recs - t * T); };
    __syncthreads();  // LDS tables are set up
    if (tile < n_tiles) {
        load_offsets(tile);
        if (tid <= T) toffs[tid] = off_a;
        __syncthreads();
        stage_tile_dma(P.recs, recs_limit, toffs, tile_count(tile), pieces, stage, tid);
        if (tile + tstride < n_tiles) load_offsets(tile + tstride);
    }

    for (uint32_t it = 0; tile < n_tiles; tile += tstride, it++) {
        const uint32_t par = it & 1u;
        const uint32_t *cur_offs = toffs + par * TOFF;
        const uint32_t r0 = tile * T;
        const uint32_t count = min(T, n_recs - r0);
        const uint32_t next = tile + tstride;

        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // DMA pieces + offset loads of this wave are in
        if (next < n_tiles && tid <= T) toffs[(par ^ 1u) * TOFF + tid] = off_a;  // next tile's offsets
        __syncthreads();  // everyone's DMA landed; previous COLUMNS pass is over

        // ---- CODES, part A: everything that reads `stage` ---------------------------------------
        // A lane pair per read (TILED_MAX_T * 2 == TILED_THREADS: one (read, end) per thread).
        // e = 0: left alignment end, 1: right end.
        const uint32_t j = tid >> 1, e = tid & 1u;
        const bool lane_on = tid < 2u * T && !(ablate & 4u);
        const bool in_tile = lane_on && j < count;
        uint32_t o0 = 0, o1 = 0;
        if (in_tile) { o0 = cur_offs[j]; o1 = cur_offs[j + 1]; }
        // record j's first `pieces` 16-byte pieces sit at stage + j*pieces*16, starting at its
        // 16-byte aligned address: byte x of the record is at offset (o0 & 15) + x
        const uint32_t avail = pieces * 16u - (o0 & 15u);       // record bytes present in LDS
        const bool hdr_ok = in_tile && o1 - o0 >= 36u && avail >= 48u;
        // lanes without a usable record decode a harmless dummy (offset 0, length 0 -> malformed ->
        // dead) so the lanes of a wave stay on one path
        LdsBytes src{stage, hdr_ok ? j * pieces * 16u + (o0 & 15u) : 0u};
        const RecHdr h = decode_hdr_lds(src, hdr_ok ? o1 - o0 : 0u);
        // everything the path reads ends at QUAL[0] (the -R filter and -G walk the aux fields: whole record;
        // a length bin needs nothing behind QUAL[0]; -Q and the read score read QUAL to its end)
        const uint32_t needed = (PLANES == PLANES_RG || P.rg) ? o1 - o0 : (MASKQ || SCORE) ? h.aux_off : h.qual_off + 1u;
        // (-I: a CIGAR of more ops than a lane walks sends the record to the one-lane path)
        bool in_stage = GAPPED ? hdr_ok && needed <= avail && h.n_cigar <= GAPPED_TILED_OPS : hdr_ok && needed <= avail;
        auto pl = plan_head<DO_PSS, DO_KMER, true, GAPPED>(P, src, h, RefsLdsCached{refs_lds, P.ref_info, n_ref_cached, (uint32_t)P.n_ref},
                                                           GAPPED && in_stage ? GAPPED_TILED_OPS : 0u);
        if constexpr (GAPPED) {
            // -I: a lane reads ONE run of read bases, the one at its own end.  A candidate with a gap whose other run begins
            // inside this end's N positions (L - b < N on the left, L - a < N on the right: every I / D of the read lies within N
            // reference bases of one end) has positions that are read through the other end's anchor: the one-lane path takes it.
            if (pl.pss_cand && pl.a != pl.L && (pl.L - pl.b < (uint32_t)N || pl.L - pl.a < (uint32_t)N)) in_stage = false;
        }
        if (!in_stage) { pl.status = RS_LIVE; pl.live = pl.pss_cand = pl.fk5 = pl.fk3 = false; }
        // this end's reference window, issued for every candidate before the -U/-D test so the
        // test costs no extra memory round trip
        const bool cand = DO_PSS && pl.pss_cand;
        // -T: the contig's region descriptor, first of the lookup's dependent loads
        const bool rcand = REGIONS && (pl.pss_cand || pl.fk5 || pl.fk3);
        uint4 rdesc = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (REGIONS) {
            if (rcand) rdesc = P.region_info[region_ref_index(P, h)];
        }
        // 32 window positions = 16 bytes of the 4-bit packed reference (+ up to 7 nibbles of
        // misalignment): five dwords, one dwordx4 + one dword gather
        uint32_t gq[5] = {0u, 0u, 0u, 0u, 0u};
        uint32_t gsh = 0u;
        uint32_t nb_front = 4u, nb_behind = 4u;   // SITE: the reference nibbles next to the window, positions -1 and 32 of it
        if (cand) {
            const uint64_t ga = pl.gbase + (uint64_t)pl.s + (e ? (uint64_t)pl.L - 30ull - row_base : (uint64_t)row_base - 2ull);
            const uint32_t *pg = P.genome4 + (ga >> 3);
            if (!(ablate & 128u)) {
                const Quad q0 = *(const Quad *)pg;
#pragma unroll
                for (int k = 0; k < 4; k++) gq[k] = q0.v[k];
                gq[4] = pg[4];
                // (a candidate's window starts at most 31 bases in front of its contig: inside the padding between contigs)
                if constexpr (SITE) nb_front = P.genome4[(ga - 1ull) >> 3] >> (4u * (uint32_t)((ga - 1ull) & 7ull));
            }
            gsh = 4u * (uint32_t)(ga & 7ull);
        }
        // -P: the 32 reference positions outside the read at this end -- s - 32 .. s - 1 on the left, s + L .. s + L + 31 on the right --
        // gathered like the window and with it, in front of the -U/-D test: no further dependent round trip.  A candidate has
        // s >= 2 and s + L + 2 <= glen, so the five dwords start at most 37 bases in front of the contig and end at most 37 behind
        // it: inside the padding between contigs (CONTIG_PAD), whose nibbles are masked by position below.  comp_out = how many
        // of the w outside offsets lie inside the contig.
        [[maybe_unused]] uint32_t go[COMP ? 5 : 1];
        [[maybe_unused]] uint32_t gosh = 0u, comp_out = 0u;
        if constexpr (COMP) {
#pragma unroll
            for (int k = 0; k < 5; k++) go[k] = 0u;
            if (cand) {
                const uint64_t oa = pl.gbase + (uint64_t)pl.s + (e ? (uint64_t)pl.L : (uint64_t)-32ll);
                const uint32_t *po = P.genome4 + (oa >> 3);
                const Quad q1 = *(const Quad *)po;
#pragma unroll
                for (int k = 0; k < 4; k++) go[k] = q1.v[k];
                go[4] = po[4];
                gosh = 4u * (uint32_t)(oa & 7ull);
                const uint32_t glen = RefsLdsCached{refs_lds, P.ref_info, n_ref_cached, (uint32_t)P.n_ref}.get((uint32_t)h.ref_id < (uint32_t)P.n_ref ? (uint32_t)h.ref_id : (uint32_t)P.n_ref).z;
                comp_out = min(P.composition, e ? glen - ((uint32_t)pl.s + pl.L) : (uint32_t)pl.s);
            }
        }
        // the first context base of this end (position s-1 / s+L) decides -U / -D in every pass; only
        // the window of pass 0 holds it
        uint32_t cx = 0u;
        if (cand && !pass0) {
            const uint64_t pc = pl.gbase + (uint64_t)pl.s + (e ? (uint64_t)pl.L : (uint64_t)-1ll);
            cx = (P.genome4[pc >> 3] >> (4u * (uint32_t)(pc & 7ull))) & 15u;
        }
        // -W: this lane's half of the read's interior [d, n_hi) -- the left-end lane walks from d & ~7 (what lies below d is
        // masked) to the cut, the right-end lane from the cut on; like MISM it reads all of SEQ, and under -Q all of QUAL, in `stage`.
        // It stands in front of the loads of the end's own read and QUAL streams so that those registers are not live across the walk.
        [[maybe_unused]] uint32_t ipk[INTERIOR ? 8 : 1];
        [[maybe_unused]] bool i_some = false;   // the read's interior is not empty
        if constexpr (INTERIOR) {
#pragma unroll
            for (int k = 0; k < 8; k++) ipk[k] = 0u;
            const uint32_t d = P.interior - 1u;
            const uint32_t n_hi = pl.L > d ? min(pl.L - d, h.l_seq) : 0u;
            i_some = cand && n_hi > d;
            if (i_some) {
                const uint32_t lo8 = d & ~7u;
                const uint32_t cut = min(n_hi, lo8 + ((((n_hi - lo8) >> 1) + 7u) & ~7u));
                count_interior_staged<MASKQ>(P.genome4, pl.gbase + (uint64_t)pl.s, stage, src.off + h.seq_off, src.off + h.qual_off,
                                             e ? cut : lo8, e ? n_hi : cut, d, P.min_bq, ipk);
            }
        }
        // read bases of this end as a nibble stream aligned with the window bytes: stream nibble
        // b <-> read base n0 + b, n0 = -2 (left: bytes 0,1 are context, their nibbles are never
        // used) or L-30 (right).  20 bytes from SEQ as six aligned dwords, one batch.
        // (-I: the same two streams at the read-side anchors -- base q0 is the left end's position 0, base q1 - 1 the right end's)
        int32_t n0 = e ? (int32_t)pl.L - 30 - (int32_t)row_base : (int32_t)row_base - 2;
        if constexpr (GAPPED) n0 = e ? (int32_t)pl.q1 - 30 - (int32_t)row_base : (int32_t)pl.q0 - 2 + (int32_t)row_base;
        // (-I: a right end whose read bases run out far in front of the window -- a long deletion -- has n0 below -32; all its
        //  positions are blanked in CODES-B, so the two streams may start anywhere inside the record)
        const int32_t n0c = GAPPED ? max(n0, -32) : n0;
        uint32_t rr[6];
#pragma unroll
        for (int k = 0; k < 6; k++) rr[k] = 0u;
        uint32_t ssh = 0u;
        if (cand) {
            const int32_t n0a = min(n0c, (int32_t)h.l_seq);  // (past SEQ everything is blanked anyway: stay inside the record)
            const uint32_t sa = src.off + (uint32_t)((int32_t)h.seq_off + (n0a >> 1));  // arithmetic shift = floor
            const uint32_t *qs = (const uint32_t *)(stage + (sa & ~3u));
            ssh = sa & 3u;
#pragma unroll
            for (int k = 0; k < 6; k++) rr[k] = qs[k];
        }
        // -n / -N: this lane's half of the whole-read compare -- the left-end lane takes read bases 0 .. cut - 1, the right-end
        // lane cut .. min(L, l_seq) - 1 (a candidate is staged through QUAL[0], so all of SEQ is in `stage`)
        [[maybe_unused]] uint32_t mm = 0u;
        if constexpr (MISM) {
            const uint32_t n_cmp = min(pl.L, h.l_seq);
            const uint32_t cut = min(n_cmp, ((n_cmp >> 1) + 7u) & ~7u);
            if (cand) mm = count_mismatches_staged(P.genome4, pl.gbase + (uint64_t)pl.s, stage, src.off + h.seq_off, e ? cut : 0u, e ? n_cmp : cut, P.mism_tv != 0u);
        }
        // -y / -Y: this lane's half of the read's score, cut like the compare (all of SEQ and QUAL is in `stage`)
        [[maybe_unused]] int32_t sc = 0;
        if constexpr (SCORE) {
            const uint32_t n_cmp = min(pl.L, h.l_seq);
            const uint32_t cut = min(n_cmp, ((n_cmp >> 1) + 7u) & ~7u);
            if (cand) sc = read_score_staged<MASKQ>(P, pl.gbase + (uint64_t)pl.s, stage, src.off + h.seq_off, src.off + h.qual_off,
                                                    e ? cut : 0u, e ? n_cmp : cut, pl.L, pl.rev);
        }
        // -Q: the QUAL bytes of the same read bases, one byte per window position: byte b <-> QUAL[n0 + b] (left,
        // pass 0: bytes 0,1 are the last SEQ bytes and belong to the context positions, which CODES-B overwrites).
        // 32 bytes at any alignment = nine aligned dwords; n0 >= -31 and QUAL starts at least 36 bytes into the
        // record, the clamp keeps the last dword within 36 bytes of the record's end (STAGE_SLACK covers that).
        uint32_t qq[MASKQ ? 9 : 1];
        uint32_t qsh = 0u;
        if constexpr (MASKQ) {
#pragma unroll
            for (int k = 0; k < 9; k++) qq[k] = 0u;
            if (cand) {
                const int32_t n0q = min(n0c, (int32_t)h.l_seq);   // (at or past l_seq nothing is a read base: blanked in CODES-B)
                const uint32_t qa = src.off + (uint32_t)((int32_t)h.qual_off + n0q);
                const uint32_t *qp = (const uint32_t *)(stage + (qa & ~3u));
                qsh = qa & 3u;
#pragma unroll
                for (int k = 0; k < 9; k++) qq[k] = qp[k];
            }
        }
        // fragkon window of this side of the alignment, fetched now so its latency overlaps the
        // other loads: the left-end lane owns the window at s-k/2.. (5' k-mer of a forward read, 3'
        // of a reverse read), the right-end lane the one at ..s+L+k/2 (fragkon.c:152-181)
        const uint32_t kwhich = e ^ (pl.rev ? 1u : 0u);  // 0 = 5' table, 1 = 3' table
        bool kmer_try = DO_KMER && (kwhich ? pl.fk3 : pl.fk5) && !(ablate & 16u);
        uint32_t kw[3] = {0u, 0u, 0u};
        uint32_t ksh = 0u;
        if (kmer_try) {
            int64_t w5, w3;
            kmer_windows(pl, P.K, w5, w3);
            const uint64_t ka = pl.gbase + (uint64_t)(kwhich ? w3 : w5);
            const Tri kq = *(const Tri *)(P.genome4 + (ka >> 3));  // 15 window nibbles at any alignment (<= 22 of 24), one gather
#pragma unroll
            for (int k = 0; k < 3; k++) kw[k] = kq.v[k];
            ksh = 4u * (uint32_t)(ka & 7ull);
        }
        // -T: the two grid words, issued behind the window gathers (the descriptor has had their issue time to arrive)
        RegionQuery rq{};
        if constexpr (REGIONS) {
            if constexpr (GAPPED) {
                if (rcand) region_grid_load(P, h, rdesc, rq, pl.L);   // (a candidate's L is its reference span)
            } else
            if (rcand) region_grid_load(P, h, rdesc, rq);
        }
        uint32_t kplane = 0u;   // k-mer planes: the record's plane, resolved by the pair's left-end lane
        if constexpr (KPLANES) {
            if (e == 0u && (pl.fk5 || pl.fk3)) kplane = record_plane<PLANES, true>(src, h, pl, *gk);
            const uint32_t left = (uint32_t)__shfl_xor((int)kplane, 1);   // every lane takes part
            if (e) kplane = left;
        }
        if constexpr (GROUPED && !KPLANES) {
            // the read's plane slot for COLUMNS; n_slots = not in this launch (its codes go to the trash plane)
            if constexpr (EACH) {
                // -A: the slot that holds the read's reference, or the first free one, claimed; none: a miss (queued)
                if (in_tile && e == 0u) {
                    uint32_t slot = gk->n_slots;
                    if (cand) {
                        const uint32_t ref = each_plane(h, *gk);
                        for (uint32_t s = 0; s < gk->n_slots; s++) {
                            uint32_t owner = each_lds[s];
                            if (owner == EACH_EMPTY) owner = atomicCAS(&each_lds[s], EACH_EMPTY, ref);
                            if (owner == EACH_EMPTY || owner == ref) { slot = s; break; }
                        }
                        if (slot == gk->n_slots) each_lds[EACH_MISSQ + atomicAdd(&each_lds[EACH_MISS_N], 1u)] = j;
                        else each_lds[EACH_USED + slot] = it + 1u;   // (every writer of this tile stores the same value)
                    }
                    grp_lds[j] = slot;
                }
            } else
            if (in_tile && e == 0u) {
                const uint32_t slot = cand ? record_plane<PLANES>(src, h, pl, *gk) - gk->plane0 : gk->n_slots;
                grp_lds[j] = slot < gk->n_slots ? slot : gk->n_slots;
            }
        }
        uint32_t ev_over = 0u;  // events of a record handled by the out-of-line path
        if (in_tile && !in_stage && e == 0u) {
            if constexpr (KPLANES) ev_over = tally_overflow_record_kmer_planes<PLANES, LDS_KMER, REGIONS>(kernarg, gk, o0, o1, lds_kmer);
            else if constexpr (GROUPED) ev_over = tally_overflow_record_planes<PLANES, MASKQ, REGIONS>(kernarg, gk, o0, o1, table);
            else ev_over = tally_overflow_record<DO_PSS, DO_KMER, LDS_KMER, MASKQ, REGIONS, ARM>(kernarg, o0, o1, table, lds_kmer, hist_lds, site_lds, end_lds);
            if (pass0) atomicAdd(&lds_delta[ST_SLOW_PATH], 1);
        }
        // First use of the gathered registers happens HERE, before the next tile's DMA is issued:
        // vmcnt retires in order and hipcc's counted wait for these loads cannot see the
        // asm-issued DMA pieces, so a wait placed after the DMA issue would also wait for the
        // whole transfer and serialise it against CODES-B / COLUMNS.
        uint32_t W[4];  // nibble q of W[m] = window position 8m + q
#pragma unroll
        for (int m = 0; m < 4; m++) W[m] = __builtin_amdgcn_alignbit(gq[m + 1], gq[m], gsh);
#pragma unroll
        for (int k = 0; k < 2; k++) kw[k] = __builtin_amdgcn_alignbit(kw[k + 1], kw[k], ksh);
        // pin those uses here (the scheduler would otherwise sink them below the DMA issue)
#pragma unroll
        for (int m = 0; m < 4; m++) asm volatile("" : "+v"(W[m]));
        asm volatile("" : "+v"(cx));
        if constexpr (SITE) {   // window position 32 = nibble (ga & 7) of the fifth dword
            nb_front &= 15u;
            nb_behind = (gq[4] >> gsh) & 15u;
            asm volatile("" : "+v"(nb_front));
            asm volatile("" : "+v"(nb_behind));
        }
        if (DO_KMER) {
#pragma unroll
            for (int k = 0; k < 2; k++) asm volatile("" : "+v"(kw[k]));
        }
        if constexpr (MASKQ) {   // the QUAL bytes are in registers before `stage` is released to the next tile's DMA
#pragma unroll
            for (int k = 0; k < 9; k++) asm volatile("" : "+v"(qq[k]));
        }
        if constexpr (MISM) {
            // the compare's genome dwords are used up here as well; the pair's two halves make the read's count (every lane
            // takes part in the exchange), and a read beyond the limit is no candidate from here on
            asm volatile("" : "+v"(mm));
            mm += (uint32_t)__shfl_xor((int)mm, 1);
            if (mism_beyond(P, mm)) pl.pss_cand = false;
        }
        if constexpr (SCORE) {
            // likewise: the walk's loads are used up here, the pair's halves make the read's score, and a read below the
            // minimum is no candidate from here on
            asm volatile("" : "+v"(sc));
            sc += __shfl_xor(sc, 1);
            if (score_below(P, sc)) pl.pss_cand = false;
        }
        if constexpr (INTERIOR) {   // the walk's genome dwords and staged bytes are used up here as well
#pragma unroll
            for (int k = 0; k < 8; k++) asm volatile("" : "+v"(ipk[k]));
        }
        [[maybe_unused]] uint32_t OU[COMP ? 4 : 1];   // -P: nibble q of OU[m] = outside position 8m + q of the gather, first used here like W
        if constexpr (COMP) {
#pragma unroll
            for (int m = 0; m < 4; m++) {
                OU[m] = __builtin_amdgcn_alignbit(go[m + 1], go[m], gosh);
                asm volatile("" : "+v"(OU[m]));
            }
            asm volatile("" : "+v"(comp_out));
        }
        if constexpr (REGIONS) {
            // -T, resolved here for the same reason: its interval loads must not wait behind the DMA.  A candidate that
            // meets no region is filtered (PSS_FILTERED / KMER_FILTERED through record_events); its gathered windows
            // are simply not used.
            if (rcand && !region_resolve(P, rq)) {
                pl.pss_cand = pl.fk5 = pl.fk3 = false;
                kmer_try = false;
            }
        }
        __syncthreads();
        [[maybe_unused]] uint32_t n_miss = 0u;   // -A: reads of this tile that found no slot (the same in every lane)
        [[maybe_unused]] bool empty_slots = false;   // -A: this tile ends by flushing and emptying every slot (likewise)
        if constexpr (EACH) {
            n_miss = each_lds[EACH_MISS_N];
            bool full = gk->each_evict != 0u;
            uint32_t n_used = 0u;
            for (uint32_t s = 0; s < gk->n_slots; s++) {
                full = full && each_lds[s] != EACH_EMPTY;
                n_used += each_lds[EACH_USED + s] == it + 1u ? 1u : 0u;
            }
            empty_slots = n_miss != 0u || (full && n_used < gk->n_slots);
        }

        // every wave is done with `stage`: the next tile's DMA starts now (its offsets were put
        // into LDS before the barrier at the top) and lands behind the rest of CODES and COLUMNS;
        // the offsets of the tile after that go into VGPRs
        if (next < n_tiles) {
            stage_tile_dma(P.recs, recs_limit, toffs + (par ^ 1u) * TOFF, tile_count(next), pieces, stage, tid);
            if (next + tstride < n_tiles) load_offsets(next + tstride);
        }

        // ---- CODES, part B: registers only ------------------------------------------------------------
        {
            // first context base next to the alignment: left window position 1 (s-1), right position 30 (s+L)
            const uint32_t own1 = !pass0 ? cx : e ? (W[3] >> 24) & 15u : (W[0] >> 4) & 15u;
            const uint32_t other1 = (uint32_t)__shfl_xor((int)own1, 1);
            if (DO_PSS) plan_finish_pss_packed(P.acgt_ctx, pl, e ? other1 : own1, e ? own1 : other1);
            uint32_t code_w[8];
#pragma unroll
            for (int k = 0; k < 8; k++) code_w[k] = CODE_NONE * 0x01010101u;
            // this lane's end feeds: left -> fwd table on forward reads, rev table on reverse reads
            const uint32_t tsel = e ^ (pl.rev ? 1u : 0u);
            // -P: this lane's end feeds c5 when it is the read's 5' end (tsel = 0: the end that feeds the forward table) and the read
            // was added to the forward table, c3 likewise.  The 64 nibbles around the end in the order of the offsets: a left end
            // has them in genome order (the window holds s - 2 .. s + 29: two nibbles down), a right end in reverse (the window
            // holds s + L - 30 .. s + L + 1: two nibbles up, then turned round like the outside half).
            if constexpr (COMP) {
                uint32_t u[8];
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const uint32_t in_l = m < 3 ? __builtin_amdgcn_alignbit(W[m < 3 ? m + 1 : 3], W[m], 8) : W[3] >> 8;
                    const uint32_t in_r = reverse_nibbles8(m < 3 ? __builtin_amdgcn_alignbit(W[3 - m], W[m < 3 ? 2 - m : 0], 24) : W[0] << 8);
                    u[m] = e ? reverse_nibbles8(OU[3 - m]) : OU[m];
                    u[4 + m] = e ? in_r : in_l;
                }
                const bool on = cand && (tsel ? pl.pss_rev : pl.pss_fwd);
                composition_wave_add(hist_lds, P.composition, u, on ? -(int32_t)comp_out : 0, on ? (int32_t)min(P.composition, pl.L) : 0, tsel, pl.rev);
                if ((it & 8191u) == 8191u) flush_composition();   // (a tile adds at most 128 to a word)
                // (in front of the codes: the outside half's registers are free again where the code words need theirs)
            }
            bool end_hit = false;   // END: this lane's end is marked
            if (cand && (tsel ? pl.pss_rev : pl.pss_fwd) && !(ablate & 2u)) {
                // Four window positions per VALU instruction, no memory lookups: v_perm_b32 with the
                // DATA as selector is an 8-entry byte table (selectors 0-7 pick a pool byte, 8-11
                // replicate the sign of pool byte 1/3/5/7, 12 gives 0x00, >= 13 gives 0xFF).
                //   read base : selector = BAM nibble ^ 4   -> A(1)->5  C(2)->6  G(4)->0  T(8)->12
                //               pool: [0]=G [5]=A [6]=C, T is the hardware's 0x00, every other nibble
                //               lands on 0xFF (pool filler, sign replicas of bytes 1,3,5,7, or >= 13);
                //               value = (3 - idx) << 3  (complemented: T must be 0), A carries 0x80 so
                //               that selector 10 (nibble 14) replicates a set sign bit
                //   reference : selector = the packed reference's nibble: 0..3 = A C G T, 4..7 = "other"
                //               pool: [0..3] = (3 - idx) << 1, [4..7] = 0xFF
                // OR of the two = (15 - cell) << 1, the reverse-strand code; forward-strand lanes XOR
                // 0x1E to get cell << 1.  Anything invalid is 0xFF and ends, after the final & 0x3F,
                // on code 33 or 63: rows >= 32 of the count table are the trash bin.
                // Both nibble streams are split into EVEN and ODD positions (byte i of E[m] / O[m] =
                // position 8m + 2i / 8m + 2i + 1); the code sheet row keeps that order, see COLUMNS.
                uint32_t S[5];
#pragma unroll
                for (int k = 0; k < 5; k++) S[k] = __builtin_amdgcn_alignbyte(rr[k + 1], rr[k], ssh);
                // SEQ byte i holds positions 2i (high nibble), 2i+1 (low nibble) when n0 is even;
                // when n0 is odd position 2i is the LOW nibble of byte i and 2i+1 the HIGH nibble of
                // byte i+1
                const bool odd = (n0 & 1) != 0;
                const uint32_t M = 0x0F0F0F0Fu;
                const uint32_t sx = pl.rev ? 0u : 0x1E1E1E1Eu;
                const uint32_t tsel4 = tsel * 0x01010101u;
                uint32_t RE[4], RO[4], GE[4], GO[4];
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const uint32_t S1 = __builtin_amdgcn_alignbyte(S[m + 1], S[m], 1);
                    const uint32_t A = odd ? S1 : S[m];
                    const uint32_t hiA = (A >> 4) & M, loS = S[m] & M;
                    const uint32_t E = odd ? loS : hiA, O = odd ? hiA : loS;
                    RE[m] = __builtin_amdgcn_perm(0xFF1098FFu, 0xFFFFFF08u, E ^ 0x04040404u);
                    RO[m] = __builtin_amdgcn_perm(0xFF1098FFu, 0xFFFFFF08u, O ^ 0x04040404u);
                    // the packed reference is little-endian in nibbles: even positions are the low ones
                    GE[m] = __builtin_amdgcn_perm(0xFFFFFFFFu, 0x00020406u, W[m] & M);
                    GO[m] = __builtin_amdgcn_perm(0xFFFFFFFFu, 0x00020406u, (W[m] >> 4) & M);
                }
                if constexpr (MASKQ) {
                    // QUAL byte of window position 4k + b = byte b of Qb[k]; split into even and odd positions like
                    // RE / RO and compared four positions at a time.  Done before the two steps below: positions at
                    // or past l_seq are blanked whatever their mask says, and the context positions are overwritten.
                    const uint32_t q4 = P.min_bq * 0x01010101u;
                    uint32_t Qb[8];
#pragma unroll
                    for (int k = 0; k < 8; k++) Qb[k] = __builtin_amdgcn_alignbyte(qq[k + 1], qq[k], qsh);
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        RE[m] |= base_quality_mask(__builtin_amdgcn_perm(Qb[2 * m + 1], Qb[2 * m], 0x06040200u), q4);
                        RO[m] |= base_quality_mask(__builtin_amdgcn_perm(Qb[2 * m + 1], Qb[2 * m], 0x07050301u), q4);
                    }
                }
                // bases at or beyond l_seq do not exist (precondition P3): blank them.  Rare (reads
                // shorter than the window), so the whole wave skips it when no lane needs it.
                if constexpr (GAPPED) {
                    // -I: this lane's end keeps the read bases [q0, q0 + a) (left) or [q1 - b, q1) (right), and none at or
                    // beyond l_seq (a record that does not anchor may lack them, as above): window bytes lo .. hi - 1.  Bytes
                    // 0, 1 of a left lane and 30, 31 of a right lane of pass 0 are the context positions, set below.
                    // (32-bit: a staged record's l_seq, clips and runs are a few thousand at most, a candidate's L below 2^28)
                    const int32_t r_lo = e ? (int32_t)pl.q1 - (int32_t)pl.b : (int32_t)pl.q0;
                    const int32_t r_hi = min(e ? (int32_t)pl.q1 : (int32_t)pl.q0 + (int32_t)pl.a, (int32_t)h.l_seq);
                    const int32_t lo_s = r_lo - n0, hi_s = r_hi - n0;
                    const uint32_t lo = lo_s <= 0 ? 0u : lo_s >= 32 ? 32u : (uint32_t)lo_s;
                    const uint32_t hi = hi_s <= 0 ? 0u : hi_s >= 32 ? 32u : (uint32_t)hi_s;
                    if (__any(hi < (e && pass0 ? 30u : 32u) || lo > (!e && pass0 ? 2u : 0u))) {
#pragma unroll
                        for (int m = 0; m < 4; m++) {
                            // kept: bytes i of E[m] with lo <= 8m + 2i < hi, of O[m] with lo <= 8m + 2i + 1 < hi
                            const uint32_t up = hi > 8u * m ? hi - 8u * m : 0u, dn = lo > 8u * m ? lo - 8u * m : 0u;
                            const uint32_t ne = min((up + 1u) >> 1, 4u), no = min(up >> 1, 4u);
                            const uint32_t le = min((dn + 1u) >> 1, 4u), lw = min(dn >> 1, 4u);
                            RE[m] |= (ne >= 4u ? 0u : ~((1u << (8u * ne)) - 1u)) | (le >= 4u ? 0xFFFFFFFFu : (1u << (8u * le)) - 1u);
                            RO[m] |= (no >= 4u ? 0u : ~((1u << (8u * no)) - 1u)) | (lw >= 4u ? 0xFFFFFFFFu : (1u << (8u * lw)) - 1u);
                        }
                    }
                } else {
                const int32_t have_s = (int32_t)h.l_seq - n0;
                const uint32_t have = have_s <= 0 ? 0u : have_s >= 32 ? 32u : (uint32_t)have_s;
                if (__any(have < (e && pass0 ? 30u : 32u))) {
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        // bytes i of E[m] with 8m + 2i < have, of O[m] with 8m + 2i + 1 < have
                        const uint32_t left = have > 8u * m ? have - 8u * m : 0u;
                        const uint32_t ne = min((left + 1u) >> 1, 4u), no = min(left >> 1, 4u);
                        RE[m] |= ne >= 4u ? 0u : ~((1u << (8u * ne)) - 1u);
                        RO[m] |= no >= 4u ? 0u : ~((1u << (8u * no)) - 1u);
                    }
                }
                }
                // context positions carry no read base: their cell is the diagonal one of their own
                // reference base (pss-bam.c:172-184).  Left: positions 0,1 = byte 0 of E[0], O[0];
                // right: positions 30,31 = byte 3 of E[3], O[3].
                {
                    const uint32_t ml = (e || !pass0) ? 0u : 0x000000FFu, mr = (e && pass0) ? 0xFF000000u : 0u;
                    RE[0] = (RE[0] & ~ml) | ((GE[0] << 2) & ml & 0x18181818u);
                    RO[0] = (RO[0] & ~ml) | ((GO[0] << 2) & ml & 0x18181818u);
                    RE[3] = (RE[3] & ~mr) | ((GE[3] << 2) & mr & 0x18181818u);
                    RO[3] = (RO[3] & ~mr) | ((GO[3] << 2) & mr & 0x18181818u);
                }
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    code_w[2 * m] = ((RE[m] | GE[m] | tsel4) ^ sx) & 0x3F3F3F3Fu;
                    code_w[2 * m + 1] = ((RO[m] | GO[m] | tsel4) ^ sx) & 0x3F3F3F3Fu;
                }
                if constexpr (SITE) {
                    // Reference codes are A 6, C 4, G 2, T 0, other 0xFF: bits 1-2 alone tell C (10) and G (01) from the
                    // rest (11, 00).  c? / g? carry 0x02 in the bytes that hold a C / a G.  Both windows run in genome
                    // order, so the next base of an even position is the same byte of the odd word, the next base of an
                    // odd position the following byte of the even word, and the previous bases mirror that; the bytes
                    // beyond the window's edges come from nb_front / nb_behind.  In context: C followed by G, or G
                    // preceded by C.
                    const uint32_t B = 0x02020202u;
                    uint32_t cE[4], gE[5], cO[5], gO[4];   // cO[0] / gE[4]: the words in front of / behind the window
                    cO[0] = nb_front == 1u ? 0x02000000u : 0u;
                    gE[4] = nb_behind == 2u ? 0x00000002u : 0u;
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        const uint32_t yE = GE[m] & 0x06060606u, yO = GO[m] & 0x06060606u;
                        cE[m] = (yE >> 1) & ~yE & B;
                        gE[m] = yE & ~(yE >> 1) & B;
                        cO[m + 1] = (yO >> 1) & ~yO & B;
                        gO[m] = yO & ~(yO >> 1) & B;
                    }
                    // the context positions (rows 0, 1) are reference-only: never in the in-context table
                    const uint32_t ml = (e || !pass0) ? 0u : 0x000000FFu, mr = (e && pass0) ? 0xFF000000u : 0u;
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        const uint32_t keep = ~((m == 0 ? ml : 0u) | (m == 3 ? mr : 0u));
                        const uint32_t inE = (cE[m] & gO[m]) | (gE[m] & __builtin_amdgcn_alignbyte(cO[m + 1], cO[m], 3));
                        const uint32_t inO = (cO[m + 1] & __builtin_amdgcn_alignbyte(gE[m + 1], gE[m], 1)) | (gO[m] & cE[m]);
                        code_w[2 * m] |= (inE << 5) & keep;       // 0x02 -> CODE_SITE
                        code_w[2 * m + 1] |= (inO << 5) & keep;
                    }
                }
                if constexpr (END) {
                    // Row 2 + i is window position 2 + i of a left end and 29 - i of a right end; position p is byte
                    // (p & 7) >> 1 of code word 2 * (p >> 3) + (p & 1).  So rows 2, 4, 6 / 3, 5, 7 / 8 / 9 are bytes 1-3 of
                    // words 0 / 1 and byte 0 of words 2 / 3 on the left, and the byte-reversed words 7 / 6 / 5 / 4 hold them
                    // at the same places on the right.  A byte equals the wanted code when the XOR is zero; every byte is
                    // below 0x40, so + 0x7F sets bit 7 exactly in the non-zero ones without a carry between bytes.
                    const uint32_t d = P.end_depth;
                    const uint32_t want4 = (((tsel ? P.end_cell3 : P.end_cell5) << 1) | tsel) * 0x01010101u;
                    const uint32_t rows_m[4] = {(d > 0u ? 0x00008000u : 0u) | (d > 2u ? 0x00800000u : 0u) | (d > 4u ? 0x80000000u : 0u),
                                                (d > 1u ? 0x00008000u : 0u) | (d > 3u ? 0x00800000u : 0u) | (d > 5u ? 0x80000000u : 0u),
                                                d > 6u ? 0x00000080u : 0u, d > 7u ? 0x00000080u : 0u};
                    uint32_t hit = 0u;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t x = e ? __builtin_bswap32(code_w[7 - k]) : code_w[k];
                        hit |= ~((x ^ want4) + 0x7F7F7F7Fu) & rows_m[k];
                    }
                    end_hit = hit != 0u;
                }
            }
            if constexpr (END) {
                // every lane takes part in the exchange; paired records never reach the conditional tables, and a lane that
                // adds nothing holds "no count" codes, which COLUMNS leaves out whatever the flag says
                const bool other_hit = __shfl_xor((int)end_hit, 1) != 0;
                const bool unpaired = !(pl.flag & FL_PAIRED);
                if (unpaired && other_hit) {
#pragma unroll
                    for (int k = 0; k < 8; k++) code_w[k] |= CODE_END * 0x01010101u;
                }
                // reads[4], from the left-end lane (an unpaired read is added to both tables or to none); the lane that
                // feeds the forward table holds the 5' mark.  A record on the out-of-line path counted itself there.
                const bool on = e == 0u && in_stage && unpaired && pl.pss_fwd;
                const bool m5 = tsel ? other_hit : end_hit, m3 = tsel ? end_hit : other_hit;
                const unsigned long long b0 = __ballot(on), b1 = __ballot(on && m5), b2 = __ballot(on && m3), b3 = __ballot(on && m5 && m3);
                if (lane == 0u && b0) {
                    uint32_t *reads = end_lds + 32u * n_pos;
                    atomicAdd(&reads[0], (uint32_t)__popcll(b0));
                    if (b1) atomicAdd(&reads[1], (uint32_t)__popcll(b1));
                    if (b2) atomicAdd(&reads[2], (uint32_t)__popcll(b2));
                    if (b3) atomicAdd(&reads[3], (uint32_t)__popcll(b3));
                }
            }
            bool kmer_ok = true;
            if (kmer_try) {
                // bin = base-4 number of the k bases read left to right (kmer.c:184-214); for a
                // reverse-strand read the window is reverse-complemented (fragkon.c:156-160)
                uint32_t bin = 0u, bad = 0u;
#pragma unroll
                for (int t = 0; t < 16; t++) {   // K <= 15
                    if (t < P.K) {
                        const uint32_t c = (kw[t >> 3] >> (4 * (t & 7))) & 0xFu;
                        bad |= c & ~3u;
                        bin = pl.rev ? (bin | ((3u - (c & 3u)) << (2 * t))) : ((bin << 2) | (c & 3u));
                    }
                }
                kmer_ok = bad == 0u;
                if (kmer_ok && !(ablate & 8u)) {
                    if constexpr (KPLANES) kmer_plane_add<LDS_KMER>(P, *gk, kplane, kwhich, bin, lds_kmer);
                    else if (LDS_KMER) atomicAdd(&lds_kmer[(kwhich ? (1u << (2 * P.K)) : 0u) + bin], 1u);
                    else atomicAdd(&P.counters[(kwhich ? P.off_k3 : P.off_k5) + bin], 1ull);
                }
            }
            if (lane_on && !KPLANES) {  // code sheet row of read j: bytes [e*32, e*32+32)
                uint4 *dst = (uint4 *)(sheet + j * 64u + e * 32u);
                dst[0] = make_uint4(code_w[0], code_w[1], code_w[2], code_w[3]);
                dst[1] = make_uint4(code_w[4], code_w[5], code_w[6], code_w[7]);
            }
            bool kfail = false;
            if (DO_KMER) {
                // fragkon status of the read: -1 when any attempted add failed (either lane of the pair)
                const int bad = (kmer_try && !kmer_ok) ? 1 : 0;
                const int bad_other = __shfl_xor(bad, 1);  // every lane takes part in the exchange
                kfail = (bad | bad_other) != 0;
            }
            if (e == 0u && pass0) book_events(DO_PSS, DO_KMER, in_stage ? record_events(DO_PSS, DO_KMER, pl, kfail) : ev_over, lds_delta);
            // -H: both lanes of a pair hold the same decision; the left-end lane counts the read (a record that took
            // the out-of-line path counted itself there and is no candidate here)
            if constexpr (HIST) hist_wave_add(P, hist_lds, e == 0u, pl.L, pl.pss_fwd, pl.pss_rev);
            // -N: the same for the mismatch bin (P.mism_hist is the same in every lane)
            if constexpr (MISM) {
                if (P.mism_hist) mism_wave_add(P, hist_lds, e == 0u, mism_bin(P, mm), pl.pss_fwd, pl.pss_rev);
            }
            // -Y: the same for the score bin (P.score_half is the same in every lane)
            if constexpr (SCORE) {
                if (P.score_half)
                    bin_wave_add(e == 0u, score_bin(P, sc), pl.pss_fwd, pl.pss_rev,
                                 [&](uint32_t bin, bool f, bool r, uint32_t n) { score_add(P, hist_lds, bin, f, r, n); });
            }
            // -W: both lanes of a read that was added to a table hand in their halves; the left-end lane counts the read
            if constexpr (INTERIOR) {
                interior_wave_add(hist_lds, ipk, pl.pss_fwd || pl.pss_rev, pl.rev, e == 0u && i_some);
                if ((it & 8191u) == 8191u) flush_interior();
            }
        }
        // (no barrier: wave w wrote the sheet rows of reads 32w .. 32w+31 -- j = tid >> 1 -- and its
        //  COLUMNS pass below reads exactly those rows)

        // ---- COLUMNS: wave-per-read, lane = (end, window byte) -----------------------------------
        if (DO_PSS && !(ablate & 1u)) {
            // sheet byte b of an end holds window position 8*(b/8) + 2*(b%4) + (b/4)%2 (even/odd split)
            const uint32_t e = lane >> 5, b = lane & 31u;
            const uint32_t wpos = (b & 24u) + 2u * (b & 3u) + ((b >> 2) & 1u);
            const uint32_t row = e ? 31u - wpos : wpos;
            const uint32_t j0 = min(count, wave * 32u), j1 = min(count, j0 + 32u);
            if (GROUPED && row < n_live) {
                // real codes (< 32) go to the read's plane slot, the "no count" codes to the trash plane;
                // the slot is the same for the whole wave (one read per wave-iteration): a scalar offset
                const uint32_t trash_off = (gk->n_slots - 1u) * GROUP_PLANE_WORDS;
                uint32_t j = j0;
                for (; j + 8u <= j1; j += 8u) {
                    uint32_t c[8], po[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        c[u] = sheet[(j + u) * 64u + lane];
                        po[u] = __builtin_amdgcn_readfirstlane(grp_lds[j + u]) * GROUP_PLANE_WORDS;
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++) atomicAdd(&table[(c[u] << 5) + row + (c[u] < 32u ? po[u] : trash_off)], 1u);
                }
                for (; j < j1; j++) {
                    const uint32_t c = sheet[j * 64u + lane];
                    const uint32_t po = __builtin_amdgcn_readfirstlane(grp_lds[j]) * GROUP_PLANE_WORDS;
                    atomicAdd(&table[(c << 5) + row + (c < 32u ? po : trash_off)], 1u);
                }
            } else if (SITE && row < n_live) {
                // a real code (< 32) with CODE_SITE set counts a second time, in the in-context table: its half code is
                // the code without the reference base's low bit
                auto add = [&](uint32_t c) {
                    atomicAdd(&table[((c & 63u) << 5) + row], 1u);
                    if ((c & (CODE_SITE | CODE_NONE)) == CODE_SITE) atomicAdd(&site_lds[((((c >> 1) & 14u) | (c & 1u)) << 5) + row], 1u);
                };
                uint32_t j = j0;
                for (; j + 8u <= j1; j += 8u) {
                    uint32_t c[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) c[u] = sheet[(j + u) * 64u + lane];
#pragma unroll
                    for (int u = 0; u < 8; u++) add(c[u]);
                }
                for (; j < j1; j++) add(sheet[j * 64u + lane]);
            } else if (END && row < n_live) {
                // a real code (< 32) with CODE_END set counts a second time, in the conditional tables
                auto add = [&](uint32_t c) {
                    atomicAdd(&table[((c & 63u) << 5) + row], 1u);
                    if ((c & (CODE_END | CODE_NONE)) == CODE_END) atomicAdd(&end_lds[(c & 31u) * n_pos + row], 1u);
                };
                uint32_t j = j0;
                for (; j + 8u <= j1; j += 8u) {
                    uint32_t c[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) c[u] = sheet[(j + u) * 64u + lane];
#pragma unroll
                    for (int u = 0; u < 8; u++) add(c[u]);
                }
                for (; j < j1; j++) add(sheet[j * 64u + lane]);
            } else if (row < n_live) {  // (lanes of dead rows would only ever see CODE_NONE)
                uint32_t j = j0;
                for (; j + 8u <= j1; j += 8u) {
                    uint32_t c[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) c[u] = sheet[(j + u) * 64u + lane];
#pragma unroll
                    for (int u = 0; u < 8; u++) atomicAdd(&table[(c[u] << 5) + row], 1u);
                }
                for (; j < j1; j++) atomicAdd(&table[((uint32_t)sheet[j * 64u + lane] << 5) + row], 1u);
            }
        }
        if constexpr (EACH) {
            if (empty_slots) {   // (the whole workgroup takes the branch)
                // the queued reads, one lane each, from global memory into their planes of the counter block (their events
                // were booked above, from the staged copy; this tile's offsets stay in toffs until the next tile's top)
                if (tid < n_miss) {
                    const uint32_t jm = each_lds[EACH_MISSQ + tid];
                    (void)tally_overflow_record_planes<PLANES, MASKQ, REGIONS>(kernarg, gk, cur_offs[jm], cur_offs[jm + 1u], table);
                }
                __syncthreads();   // every wave's COLUMNS pass is over
                flush_slots();
                __syncthreads();   // held[] has been read
                if (tid < EACH_MAX_SLOTS) each_lds[tid] = EACH_EMPTY;
                if (tid == 0u) each_lds[EACH_MISS_N] = 0u;
            }
        }
    }

    __syncthreads();
    // Partial results leave the workgroup as plain coalesced stores into its own scratch slot;
    // reduce_partials() sums the slots afterwards.  (Flushing with global atomics instead had
    // ~1000 workgroups queue on the same few hundred counters at the same moment: 6 % of the
    // kernel's time.)
    if constexpr (KPLANES) {   // [deltas 16 | n_slots histograms of 2 * 4^k words (LDS_KMER only)]
        uint32_t *mine = P.scratch + (size_t)blockIdx.x * gk->scratch_words;
        const uint32_t n_words = LDS_KMER ? gk->n_slots * 2u * (1u << (2 * P.K)) : 0u;
        for (uint32_t i = tid; i < n_words; i += TILED_THREADS) mine[GROUP_SCRATCH_DELTA + i] = lds_kmer[i];
        if (tid < 16u) mine[tid] = tid < (uint32_t)ST_USED ? (uint32_t)lds_delta[tid] : 0u;
    } else if constexpr (EACH) {   // [deltas 16]; the held planes go to the counter block
        flush_slots();
        uint32_t *mine = P.scratch + (size_t)blockIdx.x * gk->scratch_words;
        if (tid < 16u) mine[tid] = tid < (uint32_t)ST_USED ? (uint32_t)lds_delta[tid] : 0u;
    } else if constexpr (GROUPED) {   // [deltas 16 | n_slots planes]
        uint32_t *mine = P.scratch + (size_t)blockIdx.x * gk->scratch_words;
        const uint32_t n_words = gk->n_slots * GROUP_PLANE_WORDS;
        for (uint32_t i = tid; i < n_words; i += TILED_THREADS) mine[GROUP_SCRATCH_DELTA + i] = table[i];
        if (tid < 16u) mine[tid] = tid < (uint32_t)ST_USED ? (uint32_t)lds_delta[tid] : 0u;
    } else {
    uint32_t *mine = P.scratch + (size_t)blockIdx.x * (SITE ? SITE_SCRATCH_WORDS : END ? END_SCRATCH_WORDS : SCRATCH_WORDS);
    if constexpr (SITE)   // [table | k-mer bins | deltas | in-context table]
        for (uint32_t i = tid; i < SITE_WORDS; i += TILED_THREADS) mine[SCRATCH_WORDS + i] = site_lds[i];
    if constexpr (END) {   // [table | k-mer bins | deltas | conditional tables, 32 rows per code (rows >= N + 2 are never read)]
        for (uint32_t i = tid; i < 32u * n_pos; i += TILED_THREADS) mine[SCRATCH_WORDS + (i / n_pos) * 32u + i % n_pos] = end_lds[i];
        // reads[4]: a workgroup adds its non-zero ones to the counter block itself, as -H does with its bins
        if (tid < 4u) {
            const uint32_t v = end_lds[32u * n_pos + tid];
            if (v) atomicAdd(&P.counters[P.off_end + 2u * n_pos * 16u + tid], (unsigned long long)v);
        }
    }
    for (uint32_t i = tid; i < 32u * 32u; i += TILED_THREADS) mine[i] = DO_PSS ? table[i] : 0u;
    for (uint32_t i = tid; i < 512u; i += TILED_THREADS)
        mine[SCRATCH_KMER + i] = (LDS_KMER && i < 2u * (1u << (2 * P.K))) ? lds_kmer[i] : 0u;
    if (tid < 16u) mine[SCRATCH_DELTA + tid] = tid < (uint32_t)ST_USED ? (uint32_t)lds_delta[tid] : 0u;
    }
    if constexpr (HIST) {
        // the LDS part of hf / hr: a handful of bins are non-zero (one, for a library of equal lengths), so the
        // workgroup adds those to the counter block itself -- no scratch slot, no words for reduce_partials to walk
        for (uint32_t i = tid; i < 2u * P.hist_lds_bins; i += TILED_THREADS) {
            const uint32_t v = hist_lds[i];
            if (v) atomicAdd(&P.counters[P.off_hist + (i < P.hist_lds_bins ? i : P.hist_max + 2u + (i - P.hist_lds_bins))], (unsigned long long)v);
        }
    }
    if constexpr (MISM) {
        // [mf | mr] lie in LDS as they lie in the counter block: a few bins are non-zero, the workgroup adds those itself
        for (uint32_t i = tid; i < (P.mism_hist ? 2u * (P.mism_hist + 2u) : 0u); i += TILED_THREADS) {
            const uint32_t v = hist_lds[i];
            if (v) atomicAdd(&P.counters[P.off_mism + i], (unsigned long long)v);
        }
    }
    if constexpr (SCORE) {
        // [sf | sr] lie in LDS as they lie in the counter block
        for (uint32_t i = tid; i < 4u * P.score_half; i += TILED_THREADS) {
            const uint32_t v = hist_lds[i];
            if (v) atomicAdd(&P.counters[P.off_score + i], (unsigned long long)v);
        }
    }
    flush_interior();
    flush_composition();
}


// ---------------------------------------------------------------------------------------
// tally_compact: the tiled kernel for -r N <= 16 (the tool's default is 15)
// ---------------------------------------------------------------------------------------
// Short windows leave half of tally_tiled's work on dead positions: its 32-byte windows cost
// four v_perm groups per end and one COLUMNS wave-iteration per read whatever N is, and short
// records (30-80 bp ancient-DNA reads, 138 B) no longer hide that behind their record stream:
// BASELINE config 4 ran at 17 VALU wave-instructions per read, 66 % VALU-busy, HBM half idle
// (profiles/r02_C4_before.json).  This variant keeps the pipeline (LDS-DMA staged prefixes ->
// lane pair per read -> code sheet -> column tally) and changes the window geometry:
//   * a window holds the 16 POSITIONS of an end only (two v_perm groups): left end = read bases
//     0..15 / reference s..s+15, right end = read bases L-16..L-1 / reference s+L-16..s+L-1
//     (position i from the right = byte 15-i), so both ends use the same two groups and the left
//     end's nibble stream is always even-aligned;
//   * one dwordx4 gather per end fetches its 16 positions AND its two context bases (18 nibbles
//     at any nibble alignment fit 4 dwords);
//   * the context rows (0, 1) can only take the four diagonal cells: each (read, end) lane adds
//     them with two LDS atomics into a 16-fold replicated 16-word table (lane & 15 picks the
//     replica, so the AA/CC/GG/TT skew meets at most 4 lanes per word);
//   * the code sheet row is 32 bytes, and COLUMNS takes TWO reads per wave-iteration:
//     lane = (read parity, end, byte); the count table's 32 slots per code are (end, position),
//     so the 32 lanes of a half-wave still never share a word or a bank; the two ends' slots are
//     summed when the table leaves LDS.
// The DMA issue loop addresses through an SGPR base + 32-bit lane offset (no 64-bit VALU adds)
// and saves/restores m0 around the instruction (the compiler does not model the write).
constexpr uint32_t COMPACT_MAX_ROWS = 18;     // 2 context rows + 16 positions
constexpr uint32_t CTX_REP = 16;              // replicas of the context-row cells
constexpr uint32_t CTX_WORDS = 16 * CTX_REP;  // [table 2][row 2][base 4][replica 16]
constexpr uint32_t COMPACT_TABLE_WORDS = 33 * 32;  // codes 0..31 + one trash row (5 workgroups per CU instead of 4)

// piece q of the tile -> stage + q*16, source = record's 16-byte aligned start + 16 * piece;
// `full` tiles (count == T, every piece inside the block) skip the per-lane bounds tests
__device__ __forceinline__ void stage_tile_dma32(const uint8_t *recs, uint32_t recs_limit32, const uint32_t *tile_offs,
                                                 uint32_t count, uint32_t pieces, uint8_t *stage, uint32_t tid) {
    const uint32_t n_pieces = count * pieces;
    const uint32_t lds0 = (uint32_t)(uintptr_t)stage;
    const uint32_t magic = ((1u << 20) + pieces - 1u) / pieces;   // q / pieces, exact for q < 2^13, pieces <= 64
    for (uint32_t q0 = (tid & ~63u); q0 < n_pieces; q0 += TILED_THREADS) {
        const uint32_t q = q0 + (tid & 63u);
        const uint32_t jq = (q * magic) >> 20;
        const uint32_t j = min(jq, count - 1u), pc = q - jq * pieces;
        const uint32_t a = (tile_offs[j] & ~15u) + 16u * pc;     // < 4 GiB: the block is
        if (q < n_pieces && a <= recs_limit32) {                  // recs_limit32 = readable end - 16
            const uint32_t m0v = __builtin_amdgcn_readfirstlane(lds0 + (q0 << 4));
            uint32_t keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(a), "s"(recs), "s"(m0v) : "memory");
        }
    }
}

struct LdsTableCompact {  // overflow records (one lane, global-memory decode) in the compact layout
    uint32_t *t;          // [(cell << 1) | table][32 slots]: slot = end * 16 + (row - 2); both ends are summed at the end
    uint32_t *ctx;        // [table][row][base][replica]
    __device__ __forceinline__ void add(uint32_t table, uint32_t row, uint32_t cell) const {
        if (row >= 2u) { if (row < COMPACT_MAX_ROWS) atomicAdd(&t[(((cell << 1) | table) << 5) + (row - 2u)], 1u); }
        else atomicAdd(&ctx[((table * 2u + row) * 4u + cell / 5u) * CTX_REP], 1u);   // context cells are diagonal: 0,5,10,15
    }
};

template <bool DO_KMER, bool LDS_KMER>
__device__ __attribute__((noinline)) uint32_t tally_overflow_record_compact(const TallyParams *kernarg, uint32_t o0, uint32_t o1,
                                                                            uint32_t *table, uint32_t *ctx, uint32_t *lds_kmer) {
    const TallyParams &P = *kernarg;
    GlobalBytes gsrc{P.recs + o0};
    const RecHdr gh = decode_hdr(gsrc, o1 - o0);
    const Plan gpl = make_plan<true, DO_KMER, false>(P, gsrc, gh);   // (-T launches never take tally_compact)
    if (gpl.pss_fwd || gpl.pss_rev) tally_pss_record(P, LdsTableCompact{table, ctx}, gsrc, gh, gpl);
    bool kfail = false;
    if (DO_KMER && (gpl.fk5 || gpl.fk3)) kfail = tally_kmer_record<LDS_KMER>(P, gpl, lds_kmer);
    return record_events(true, DO_KMER, gpl, kfail);
}

template <bool DO_KMER, bool LDS_KMER, int DECODE_REPS = 1, bool PLAN_ONCE = false>
__device__ __forceinline__ void tally_compact_body(const TallyParams &P, const TallyParams *kernarg,
                                                   uint8_t *__restrict__ stage, uint8_t *__restrict__ sheet,
                                                   uint32_t *__restrict__ table, uint32_t *__restrict__ toffs,
                                                   uint32_t *__restrict__ lds_kmer, int32_t *__restrict__ lds_delta,
                                                   uint4 *__restrict__ refs_lds, uint32_t *__restrict__ ctx_rep,
                                                   uint32_t *__restrict__ ovf_list, uint32_t *__restrict__ ovf_n) {
    const uint32_t T = P.reads_per_tile;
    const uint32_t n_recs = P.n_recs_dev ? *P.n_recs_dev : P.n_recs;   // device-indexed blocks: the count lives in device memory
    const uint32_t pieces = P.prefix_pieces;
    const uint32_t recs_limit32 = (uint32_t)(((P.recs_bytes + 15ull) & ~15ull) - 16ull);  // last piece start that is readable
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6;

    // -U / -D membership by packed-reference nibble, complemented form in the upper half:
    // bit n = nibble n passes, bit 16 + n = the complement of nibble n passes
    uint32_t up_tab = 0u, dn_tab = 0u;
#pragma unroll
    for (uint32_t n = 0; n < 8u; n++) {
        const uint32_t c = n < 4u ? 3u - n : n;
        const uint32_t u = n < 4u ? (P.acgt_ctx >> (2u * n)) & 1u : n & 1u, uc = c < 4u ? (P.acgt_ctx >> (2u * c)) & 1u : c & 1u;
        const uint32_t d = n < 4u ? (P.acgt_ctx >> (2u * n + 1u)) & 1u : (n >> 1) & 1u, dc = c < 4u ? (P.acgt_ctx >> (2u * c + 1u)) & 1u : (c >> 1) & 1u;
        up_tab |= (u << n) | (uc << (16u + n));
        dn_tab |= (d << n) | (dc << (16u + n));
    }

    for (uint32_t i = tid; i < COMPACT_TABLE_WORDS; i += TILED_THREADS) table[i] = 0u;
    if (tid < CTX_WORDS) ctx_rep[tid] = 0u;
    if (LDS_KMER)
        for (uint32_t i = tid; i < 2u * (1u << (2 * P.K)); i += TILED_THREADS) lds_kmer[i] = 0u;
    if (tid < ST_USED) lds_delta[tid] = 0;
    if (tid == 0u) *ovf_n = 0u;
    const uint32_t n_ref_cached = min((uint32_t)P.n_ref, REF_LDS_ENTRIES);
    if (tid < n_ref_cached) refs_lds[tid] = P.ref_info[tid];
    if (tid == n_ref_cached) refs_lds[tid] = P.ref_info[P.n_ref];
    const uint32_t all_tiles = (n_recs + T - 1u) / T;
    uint32_t tile = blockIdx.x;
    const uint32_t tstride = gridDim.x, n_tiles = all_tiles;
    uint32_t off_a = 0;
    const uint32_t TOFF = TILED_MAX_T + 4u;
    auto load_offsets = [&](uint32_t t) {
        const uint32_t r0 = t * T;
        if (tid <= T && r0 + tid <= n_recs) off_a = P.offs[r0 + tid];
    };
    auto tile_count = [&](uint32_t t) { return min(T, n_recs - t * T); };
    __syncthreads();
    if (tile < n_tiles) {
        load_offsets(tile);
        if (tid <= T) toffs[tid] = off_a;
        __syncthreads();
        stage_tile_dma32(P.recs, recs_limit32, toffs, tile_count(tile), pieces, stage, tid);
        if (tile + tstride < n_tiles) load_offsets(tile + tstride);
    }

    for (uint32_t it = 0; tile < n_tiles; tile += tstride, it++) {
        const uint32_t par = it & 1u;
        const uint32_t *cur_offs = toffs + par * TOFF;
        const uint32_t r0 = tile * T;
        const uint32_t count = min(T, n_recs - r0);
        const uint32_t next = tile + tstride;

        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (next < n_tiles && tid <= T) toffs[(par ^ 1u) * TOFF + tid] = off_a;
        __syncthreads();

        // ---- CODES, part A: everything that reads `stage` --------------------------------------
        const uint32_t j = tid >> 1, e = tid & 1u;
        const bool lane_on = tid < 2u * T;
        Plan pl;
        uint32_t l_seq = 0, soff = 0;   // SEQ length; LDS offset of the SEQ bytes of the staged record
        bool in_stage = false;
        if constexpr (PLAN_ONCE) {
            // A1: ONE lane per read (waves 0 and 1 of the four) decodes the header and applies the filters; the plan -- eight
            // words -- goes to LDS, where the code sheet will be written later (free between the previous tile's COLUMNS and
            // this tile's part B), and after one more barrier BOTH lanes of the read's pair pick it up.  The pair used to do
            // all of this twice, side by side: 17.6 % of the kernel's time on C4 (tools/ab_decode_twice.sh).
            uint4 *plan_lds = (uint4 *)sheet;
            if (tid < T) {
                const bool in_t = tid < count;
                uint32_t o0 = 0, o1 = 0;
                if (in_t) { o0 = cur_offs[tid]; o1 = cur_offs[tid + 1]; }
                const uint32_t avail = pieces * 16u - (o0 & 15u);
                const bool hdr_ok = in_t && o1 - o0 >= 36u && avail >= 48u;
                LdsBytes src{stage, hdr_ok ? tid * pieces * 16u + (o0 & 15u) : 0u};
                const RecHdr h = decode_hdr_lds32(src, hdr_ok ? o1 - o0 : 0u);
                const bool staged = hdr_ok && h.qual_off + 1u <= avail;
                Plan p1 = plan_head<true, DO_KMER, false>(P, src, h, RefsLdsCached{refs_lds, P.ref_info, n_ref_cached, (uint32_t)P.n_ref});
                if (!staged) { p1.status = RS_LIVE; p1.live = p1.pss_cand = p1.fk5 = p1.fk3 = false; }
                if (in_t && !staged) ovf_list[atomicAdd(ovf_n, 1u)] = tid;   // handled behind COLUMNS (below)
                const uint32_t bits = (p1.flag & 0xFFFFu) | (p1.status << 16) | (p1.live ? 1u << 18 : 0u) | (p1.pss_cand ? 1u << 19 : 0u) |
                                      (p1.fk5 ? 1u << 20 : 0u) | (p1.fk3 ? 1u << 21 : 0u) | (staged ? 1u << 22 : 0u);
                plan_lds[2u * tid] = make_uint4((uint32_t)p1.gbase, (uint32_t)(p1.gbase >> 32), (uint32_t)p1.s, p1.L);
                plan_lds[2u * tid + 1u] = make_uint4(h.l_seq, src.off + h.seq_off, bits, p1.Lk);
            }
            __syncthreads();
            const uint4 qa = plan_lds[2u * j], qb = plan_lds[2u * j + 1u];   // (j < 128: inside the sheet whatever T is)
            pl.gbase = (uint64_t)qa.x | ((uint64_t)qa.y << 32);
            pl.s = (int32_t)qa.z;
            pl.L = qa.w;
            l_seq = qb.x;
            soff = qb.y;
            pl.flag = qb.z & 0xFFFFu;
            pl.status = (qb.z >> 16) & 3u;
            pl.live = lane_on && ((qb.z >> 18) & 1u);
            pl.pss_cand = lane_on && ((qb.z >> 19) & 1u);
            pl.fk5 = lane_on && ((qb.z >> 20) & 1u);
            pl.fk3 = lane_on && ((qb.z >> 21) & 1u);
            in_stage = lane_on && ((qb.z >> 22) & 1u);
            pl.Lk = qb.w;
            pl.rev = (pl.flag & FL_REVERSE) != 0;
            pl.pss_fwd = pl.pss_rev = false;
        } else {
        const bool in_tile = lane_on && j < count;
        uint32_t o0 = 0, o1 = 0;
        if (in_tile) { o0 = cur_offs[j]; o1 = cur_offs[j + 1]; }
        const uint32_t avail = pieces * 16u - (o0 & 15u);
        const bool hdr_ok = in_tile && o1 - o0 >= 36u && avail >= 48u;
        LdsBytes src{stage, hdr_ok ? j * pieces * 16u + (o0 & 15u) : 0u};
        const RecHdr h = decode_hdr_lds32(src, hdr_ok ? o1 - o0 : 0u);
        const uint32_t needed = h.qual_off + 1u;   // (the -R filter, which walks the aux fields, stays with tally_tiled)
        in_stage = hdr_ok && needed <= avail;
        pl = plan_head<true, DO_KMER, false>(P, src, h, RefsLdsCached{refs_lds, P.ref_info, n_ref_cached, (uint32_t)P.n_ref});
        if constexpr (DECODE_REPS > 1) {
            // diagnostics (PSSBAM_COMPACT_DECODE_TWICE): header decode + filters a second time, from an offset the
            // compiler cannot tell from the first -- the time this adds is what the pair's shared decode costs per tile
            uint32_t off2 = src.off;
            asm volatile("" : "+v"(off2));
            const LdsBytes src2{stage, off2};
            const RecHdr h2 = decode_hdr_lds32(src2, hdr_ok ? o1 - o0 : 0u);
            const Plan p2 = plan_head<true, DO_KMER, false>(P, src2, h2, RefsLdsCached{refs_lds, P.ref_info, n_ref_cached, (uint32_t)P.n_ref});
            const uint32_t sink = (uint32_t)p2.s ^ p2.L ^ p2.flag ^ (uint32_t)p2.gbase ^ (uint32_t)(p2.gbase >> 32) ^ p2.status ^ (p2.pss_cand ? 1u : 0u) ^
                                  (p2.rev ? 2u : 0u) ^ (p2.fk5 ? 4u : 0u) ^ (p2.fk3 ? 8u : 0u) ^ h2.seq_off ^ h2.qual_off;
            asm volatile("" ::"v"(sink));
        }
        if (!in_stage) { pl.status = RS_LIVE; pl.live = pl.pss_cand = pl.fk5 = pl.fk3 = false; }
        l_seq = h.l_seq;
        soff = src.off + h.seq_off;
        // a record whose needed prefix is not staged is queued and handled after COLUMNS, where
        // almost nothing is live (the out-of-line call would otherwise sit in the register-hungry
        // middle of the tile)
        if (in_tile && !in_stage && e == 0u) ovf_list[atomicAdd(ovf_n, 1u)] = j;
        }
        const bool cand = pl.pss_cand;
        // this end's 16 positions + 2 context bases: 18 nibbles of the packed reference from
        //   left : s-2 .. s+15      (nibbles 0,1 = second, first context base; 2..17 = positions 0..15)
        //   right: s+L-16 .. s+L+1  (nibbles 0..15 = positions, byte w <-> position 15-w from the
        //                            right end; 16, 17 = first, second context base)
        uint32_t gq[4] = {0u, 0u, 0u, 0u};
        uint32_t gsh = 0u;
        if (cand) {
            const uint64_t ga = pl.gbase + (uint64_t)(int64_t)((int32_t)pl.s + (e ? (int32_t)pl.L - 16 : -2));
            const Quad q0 = *(const Quad *)(P.genome4 + (ga >> 3));
#pragma unroll
            for (int k = 0; k < 4; k++) gq[k] = q0.v[k];
            gsh = 4u * (uint32_t)(ga & 7ull);
        }
        // read bases as a nibble stream aligned with the window bytes: stream nibble b <-> read base
        // n0 + b, n0 = 0 (left) or L-16 (right; may be negative for L < 16: those positions are
        // beyond N <= L and never tallied).  9 bytes at any byte alignment = three aligned dwords.
        const int32_t n0 = e ? (int32_t)pl.L - 16 : 0;
        uint32_t rr[3] = {0u, 0u, 0u};
        uint32_t ssh = 0u;
        if (cand) {
            const int32_t n0a = min(n0, (int32_t)l_seq);
            const uint32_t sa = soff + (uint32_t)(n0a >> 1);
            const uint32_t *qs = (const uint32_t *)(stage + (sa & ~3u));
            ssh = sa & 3u;
#pragma unroll
            for (int k = 0; k < 3; k++) rr[k] = qs[k];
        }
        const uint32_t kwhich = e ^ (pl.rev ? 1u : 0u);
        const bool kmer_try = DO_KMER && (kwhich ? pl.fk3 : pl.fk5);
        uint32_t kw[3] = {0u, 0u, 0u};
        uint32_t ksh = 0u;
        if (kmer_try) {
            int64_t w5, w3;
            kmer_windows(pl, P.K, w5, w3);
            const uint64_t ka = pl.gbase + (uint64_t)(kwhich ? w3 : w5);
            const Tri kq = *(const Tri *)(P.genome4 + (ka >> 3));
#pragma unroll
            for (int k = 0; k < 3; k++) kw[k] = kq.v[k];
            ksh = 4u * (uint32_t)(ka & 7ull);
        }
        // consume the gathered registers before the next DMA is issued (vmcnt retires in order)
        uint32_t A[3];  // nibble q of A[m] = window nibble 8m + q
#pragma unroll
        for (int m = 0; m < 3; m++) A[m] = __builtin_amdgcn_alignbit(gq[m + 1], gq[m], gsh);
#pragma unroll
        for (int k = 0; k < 2; k++) kw[k] = __builtin_amdgcn_alignbit(kw[k + 1], kw[k], ksh);
#pragma unroll
        for (int m = 0; m < 3; m++) asm volatile("" : "+v"(A[m]));
        if (DO_KMER) {
#pragma unroll
            for (int k = 0; k < 2; k++) asm volatile("" : "+v"(kw[k]));
        }
        __syncthreads();

        if (next < n_tiles) {
            stage_tile_dma32(P.recs, recs_limit32, toffs + (par ^ 1u) * TOFF, tile_count(next), pieces, stage, tid);
            if (next + tstride < n_tiles) load_offsets(next + tstride);
        }

        // ---- CODES, part B: registers only -----------------------------------------------------
        {
            // context nibbles: left = nibbles 0 (second), 1 (first) of A[0]; right = nibbles 0 (first), 1 (second) of A[2]
            const uint32_t cx = e ? A[2] : A[0];
            const uint32_t c_lo = cx & 15u, c_hi = (cx >> 4) & 15u;
            const uint32_t own1 = e ? c_lo : c_hi, own2 = e ? c_hi : c_lo;   // first / second context base of this end
            const uint32_t other1 = (uint32_t)__shfl_xor((int)own1, 1);
            {   // pss-bam.c:134-142, :428-494 with the membership tables
                const uint32_t left1 = e ? other1 : own1, right1 = e ? own1 : other1;
                const uint32_t rsh = pl.rev ? 16u : 0u;
                const bool up_ok = ((up_tab >> ((pl.rev ? right1 : left1) + rsh)) & 1u) != 0;
                const bool dn_ok = ((dn_tab >> ((pl.rev ? left1 : right1) + rsh)) & 1u) != 0;
                const bool paired = (pl.flag & FL_PAIRED) != 0;
                const bool r1 = (pl.flag & FL_READ1) != 0, r2 = (pl.flag & FL_READ2) != 0;
                pl.pss_fwd = pl.pss_cand && (paired ? (r1 && up_ok) : (up_ok && dn_ok));
                pl.pss_rev = pl.pss_cand && (paired ? (!(r1 && up_ok) && r2 && dn_ok) : (up_ok && dn_ok));
            }
            // the 16 position nibbles: left = window nibbles 2..17, right = 0..15
            const uint32_t G0 = e ? A[0] : __builtin_amdgcn_alignbit(A[1], A[0], 8);
            const uint32_t G1 = e ? A[1] : __builtin_amdgcn_alignbit(A[2], A[1], 8);
            uint32_t code_w[4];
#pragma unroll
            for (int k = 0; k < 4; k++) code_w[k] = CODE_NONE * 0x01010101u;
            const uint32_t tsel = e ^ (pl.rev ? 1u : 0u);
            const bool tallied = cand && (tsel ? pl.pss_rev : pl.pss_fwd);
            if (tallied) {
                // (same v_perm byte tables as tally_tiled, two groups)
                uint32_t S[3];
                S[0] = __builtin_amdgcn_alignbyte(rr[1], rr[0], ssh);
                S[1] = __builtin_amdgcn_alignbyte(rr[2], rr[1], ssh);
                S[2] = __builtin_amdgcn_alignbyte(0u, rr[2], ssh);
                const bool odd = (n0 & 1) != 0;
                const uint32_t M = 0x0F0F0F0Fu;
                const uint32_t sx = pl.rev ? 0u : 0x1E1E1E1Eu;
                const uint32_t tsel4 = tsel * 0x01010101u;
                const uint32_t Gw[2] = {G0, G1};
                uint32_t RE[2], RO[2], GE[2], GO[2];
#pragma unroll
                for (int m = 0; m < 2; m++) {
                    const uint32_t S1 = __builtin_amdgcn_alignbyte(S[m + 1], S[m], 1);
                    const uint32_t Ax = odd ? S1 : S[m];
                    const uint32_t hiA = (Ax >> 4) & M, loS = S[m] & M;
                    const uint32_t E = odd ? loS : hiA, O = odd ? hiA : loS;
                    RE[m] = __builtin_amdgcn_perm(0xFF1098FFu, 0xFFFFFF08u, E ^ 0x04040404u);
                    RO[m] = __builtin_amdgcn_perm(0xFF1098FFu, 0xFFFFFF08u, O ^ 0x04040404u);
                    GE[m] = __builtin_amdgcn_perm(0xFFFFFFFFu, 0x00020406u, Gw[m] & M);
                    GO[m] = __builtin_amdgcn_perm(0xFFFFFFFFu, 0x00020406u, (Gw[m] >> 4) & M);
                }
                // bases at or beyond l_seq do not exist (precondition P3): blank them
                const int32_t have_s = (int32_t)l_seq - n0;
                const uint32_t have = have_s <= 0 ? 0u : have_s >= 16 ? 16u : (uint32_t)have_s;
                if (__any(have < 16u)) {
#pragma unroll
                    for (int m = 0; m < 2; m++) {
                        const uint32_t left = have > 8u * m ? have - 8u * m : 0u;
                        const uint32_t ne = min((left + 1u) >> 1, 4u), no = min(left >> 1, 4u);
                        RE[m] |= ne >= 4u ? 0u : ~((1u << (8u * ne)) - 1u);
                        RO[m] |= no >= 4u ? 0u : ~((1u << (8u * no)) - 1u);
                    }
                }
#pragma unroll
                for (int m = 0; m < 2; m++) {
                    code_w[2 * m] = ((RE[m] | GE[m] | tsel4) ^ sx) & 0x3F3F3F3Fu;
                    code_w[2 * m + 1] = ((RO[m] | GO[m] | tsel4) ^ sx) & 0x3F3F3F3Fu;
                }
                // context rows (pss-bam.c:169-189): row 1 <- first context base, row 0 <- second; the
                // cell is the diagonal one of the base (complemented for reverse-strand reads)
                const uint32_t rep = lane & (CTX_REP - 1u);
                const uint32_t b1 = pl.rev ? 3u - own1 : own1, b2 = pl.rev ? 3u - own2 : own2;
                if (own1 < 4u) atomicAdd(&ctx_rep[((tsel * 2u + 1u) * 4u + b1) * CTX_REP + rep], 1u);
                if (own2 < 4u) atomicAdd(&ctx_rep[((tsel * 2u + 0u) * 4u + b2) * CTX_REP + rep], 1u);
            }
            bool kmer_ok = true;
            if (kmer_try) {
                uint32_t bin = 0u, bad = 0u;
#pragma unroll
                for (int t = 0; t < 16; t++) {   // K <= 15
                    if (t < P.K) {
                        const uint32_t c = (kw[t >> 3] >> (4 * (t & 7))) & 0xFu;
                        bad |= c & ~3u;
                        bin = pl.rev ? (bin | ((3u - (c & 3u)) << (2 * t))) : ((bin << 2) | (c & 3u));
                    }
                }
                kmer_ok = bad == 0u;
                if (kmer_ok) {
                    if (LDS_KMER) atomicAdd(&lds_kmer[(kwhich ? (1u << (2 * P.K)) : 0u) + bin], 1u);
                    else atomicAdd(&P.counters[(kwhich ? P.off_k3 : P.off_k5) + bin], 1ull);
                }
            }
            if (lane_on)   // code sheet row of read j: 16 bytes per end, [E0 O0 E1 O1]
                *(uint4 *)(sheet + j * 32u + e * 16u) = make_uint4(code_w[0], code_w[1], code_w[2], code_w[3]);
            bool kfail = false;
            if (DO_KMER) {
                const int bad = (kmer_try && !kmer_ok) ? 1 : 0;
                const int bad_other = __shfl_xor(bad, 1);
                kfail = (bad | bad_other) != 0;
            }
            if (e == 0u && in_stage) book_events(true, DO_KMER, record_events(true, DO_KMER, pl, kfail), lds_delta);
        }
        // (no barrier here: wave w wrote the sheet rows of reads 32w .. 32w+31 -- j = tid >> 1 -- and
        //  its COLUMNS pass reads exactly those rows)

        // ---- COLUMNS: two reads per wave-iteration, lane = (read parity, end, sheet byte) ----------
        {
            // sheet byte b of an end holds window byte w = 8*(b/8) + 2*(b%4) + (b/4)%2; left: position w,
            // right: position 15-w; table slot = end*16 + position.  Every code >= 32 ("no count")
            // lands in the one trash row 32.
            const uint32_t ee = (lane >> 4) & 1u, b = lane & 15u;
            const uint32_t w = (b & 8u) + 2u * (b & 3u) + ((b >> 2) & 1u);
            const uint32_t posn = ee ? 15u - w : w;
            const uint32_t slot = ee * 16u + posn;
            const uint32_t j0 = min(count, wave * 32u), j1 = min(count, j0 + 32u);
            if (posn < (uint32_t)P.N) {
                const uint32_t rd = lane >> 5;   // which read of the pair
                uint32_t jj = j0;
                for (; jj + 16u <= j1; jj += 16u) {
                    uint32_t c[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) c[u] = sheet[(jj + 2u * u) * 32u + lane];
#pragma unroll
                    for (int u = 0; u < 8; u++) atomicAdd(&table[(min(c[u], 32u) << 5) + slot], 1u);
                }
                for (; jj < j1; jj += 2u)
                    if (jj + rd < j1) atomicAdd(&table[(min((uint32_t)sheet[jj * 32u + lane], 32u) << 5) + slot], 1u);
            }
        }
        // queued overflow records of this tile (rare: a record of tens of KB, or a block whose later
        // records are longer than the sampled prefix).  ovf_n was final at the barrier behind CODES-A.
        const uint32_t n_ovf = *ovf_n;
        if (n_ovf) {
            for (uint32_t i = tid; i < n_ovf; i += TILED_THREADS) {
                const uint32_t jo = ovf_list[i];
                const uint32_t ev = tally_overflow_record_compact<DO_KMER, LDS_KMER>(kernarg, cur_offs[jo], cur_offs[jo + 1u], table,
                                                                                    ctx_rep, lds_kmer);
                book_events(true, DO_KMER, ev, lds_delta);
                atomicAdd(&lds_delta[ST_SLOW_PATH], 1);
            }
            __syncthreads();   // everyone has read n_ovf / the list
            if (tid == 0u) *ovf_n = 0u;
        }
    }

    __syncthreads();
    // scratch slot in tally_tiled's format ([code][row]): rows 2.. = both ends' slots summed,
    // rows 0,1 = the context replicas summed (diagonal cells only)
    uint32_t *mine = P.scratch + (size_t)blockIdx.x * SCRATCH_WORDS;
    for (uint32_t i = tid; i < 32u * 32u; i += TILED_THREADS) {
        const uint32_t ct = i >> 5, row = i & 31u;
        uint32_t v = 0u;
        if (row >= 2u && row < COMPACT_MAX_ROWS) v = table[(ct << 5) + (row - 2u)] + table[(ct << 5) + 16u + (row - 2u)];
        else if (row < 2u) {
            const uint32_t t = ct & 1u, cell = ct >> 1;
            if (cell % 5u == 0u) {
                const uint32_t *rp = ctx_rep + ((t * 2u + row) * 4u + cell / 5u) * CTX_REP;
                for (uint32_t k = 0; k < CTX_REP; k++) v += rp[k];
            }
        }
        mine[i] = v;
    }
    for (uint32_t i = tid; i < 512u; i += TILED_THREADS)
        mine[SCRATCH_KMER + i] = (LDS_KMER && i < 2u * (1u << (2 * P.K))) ? lds_kmer[i] : 0u;
    if (tid < 16u) mine[SCRATCH_DELTA + tid] = tid < (uint32_t)ST_USED ? (uint32_t)lds_delta[tid] : 0u;
}

template <bool DO_KMER, bool LDS_KMER, bool PLAN_ONCE = false>
__global__ void __launch_bounds__(TILED_THREADS) tally_compact(const TallyParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    __shared__ __attribute__((aligned(16))) uint8_t sheet[TILED_MAX_T * 32u];
    __shared__ uint32_t table[COMPACT_TABLE_WORDS];
    __shared__ uint32_t toffs[2u * (TILED_MAX_T + 4u)];
    __shared__ uint32_t lds_kmer[LDS_KMER ? 2u * (1u << (2 * KMER_LDS_MAX_K)) : 1u];
    __shared__ int32_t lds_delta[ST_USED];
    __shared__ uint4 refs_lds[REF_LDS_ENTRIES + 1];
    __shared__ uint32_t ctx_rep[CTX_WORDS];
    __shared__ uint32_t ovf_list[TILED_MAX_T + 1];   // [TILED_MAX_T] = fill count
    const TallyParams *kernarg = (const TallyParams *)__builtin_amdgcn_kernarg_segment_ptr();
    tally_compact_body<DO_KMER, LDS_KMER, 1, PLAN_ONCE>(P, kernarg, stage, sheet, table, toffs, lds_kmer, lds_delta, refs_lds, ctx_rep, ovf_list,
                                                        ovf_list + TILED_MAX_T);
}

// diagnostics only (PSSBAM_COMPACT_DECODE_TWICE): the same kernel with the header decode + filters done twice per lane
__global__ void __launch_bounds__(TILED_THREADS) tally_compact_decode_twice(const TallyParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    __shared__ __attribute__((aligned(16))) uint8_t sheet[TILED_MAX_T * 32u];
    __shared__ uint32_t table[COMPACT_TABLE_WORDS];
    __shared__ uint32_t toffs[2u * (TILED_MAX_T + 4u)];
    __shared__ uint32_t lds_kmer[1u];
    __shared__ int32_t lds_delta[ST_USED];
    __shared__ uint4 refs_lds[REF_LDS_ENTRIES + 1];
    __shared__ uint32_t ctx_rep[CTX_WORDS];
    __shared__ uint32_t ovf_list[TILED_MAX_T + 1];
    const TallyParams *kernarg = (const TallyParams *)__builtin_amdgcn_kernarg_segment_ptr();
    tally_compact_body<false, false, 2>(P, kernarg, stage, sheet, table, toffs, lds_kmer, lds_delta, refs_lds, ctx_rep, ovf_list,
                                        ovf_list + TILED_MAX_T);
}

// Sums the per-workgroup partials of one tally_tiled launch into the u64 counter block.
// Thread (word w, group g) adds up slots g, g+REDUCE_GROUPS, ... of word w (loads coalesce across
// w) and contributes one atomic; launched on the same stream right behind the tally kernel.
// SITE: the slots of a SITE launch, SITE_SCRATCH_WORDS apart; word SCRATCH_WORDS + (half code << 5 | row) goes to
// the [fwd_in | rev_in] pair at P.off_site (rows 0 and 1 of the pair are never written).
// END: the slots of an END launch, END_SCRATCH_WORDS apart; word SCRATCH_WORDS + (code << 5 | row) goes to the
// [fwd_c | rev_c] pair at P.off_end.
constexpr uint32_t REDUCE_GROUPS = 32;
template <bool SITE = false, bool END = false>
__global__ void __launch_bounds__(256) reduce_partials(const TallyParams P, uint32_t n_slots, uint32_t lds_kmer_on) {
    constexpr uint32_t SLOT_WORDS = SITE ? SITE_SCRATCH_WORDS : END ? END_SCRATCH_WORDS : SCRATCH_WORDS;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = gid % SLOT_WORDS, g = gid / SLOT_WORDS;
    if (g >= REDUCE_GROUPS) return;
    const bool do_pss = (P.tally_mask & 1u) != 0, do_kmer = (P.tally_mask & 2u) != 0;
    const uint32_t n_pos = (uint32_t)P.N + 2u;
    unsigned long long *dst = nullptr;
    bool is_delta = false;
    if (i < 1024u) {
        const uint32_t row = P.row_base + (i & 31u), ct = i >> 5, t = ct & 1u, cell = ct >> 1;
        if (do_pss && row < n_pos) dst = &P.counters[(t ? P.off_rev : 0u) + row * 16u + cell];
    } else if (i < SCRATCH_DELTA) {
        const uint32_t k = i - SCRATCH_KMER, nb = do_kmer ? 1u << (2 * P.K) : 0u;
        if (lds_kmer_on && k < 2u * nb) dst = &P.counters[k < nb ? P.off_k5 + k : P.off_k3 + (k - nb)];
    } else if (SITE && i >= SCRATCH_WORDS) {
        const uint32_t k = i - SCRATCH_WORDS, row = P.row_base + (k & 31u), hc = k >> 5;
        const uint32_t cell = ((hc >> 2) << 2) | ((hc & 2u) ? 2u : 1u);
        if (row >= 2u && row < n_pos) dst = &P.counters[P.off_site + ((hc & 1u) ? n_pos * 16u : 0u) + row * 16u + cell];
    } else if (END && i >= SCRATCH_WORDS) {
        const uint32_t k = i - SCRATCH_WORDS, row = k & 31u, ct = k >> 5;
        if (row < n_pos) dst = &P.counters[P.off_end + ((ct & 1u) ? n_pos * 16u : 0u) + row * 16u + (ct >> 1)];
    } else {
        const uint32_t k = i - SCRATCH_DELTA;  // status counters belong to pass 0
        if (k < (uint32_t)ST_USED && P.row_base == 0u) { dst = &P.counters[P.off_stats + k]; is_delta = true; }
    }
    if (!dst) return;
    long long sum = 0;
    const uint32_t *p = P.scratch + i;
#pragma unroll 8
    for (uint32_t b = g; b < n_slots; b += REDUCE_GROUPS) {
        const uint32_t v = p[(size_t)b * SLOT_WORDS];
        sum += is_delta ? (long long)(int32_t)v : (long long)v;
    }
    if (is_delta && g == 0u) {
        // every launch credits its record count to the OK slots; the deltas move records elsewhere
        const uint32_t k = i - SCRATCH_DELTA;
        if (k == ST_RECORDS || (do_pss && k == ST_PSS_OK) || (do_kmer && k == ST_KMER_OK)) sum += P.n_recs_dev ? *P.n_recs_dev : P.n_recs;
    }
    if (sum) atomicAdd(dst, (unsigned long long)sum);
}

// Dynamic LDS is the staging buffer and, behind it, what the arm keeps there (hist_lds; never two arms at once):
// HIST: the 2 * P.hist_lds_bins words of the length histogram
// SITE: nothing there; one more static object, the 2 KiB in-context table
// END: the conditional tables and reads[4], end_lds_bytes(N + 2)
// GAPPED: nothing more in LDS (the CIGAR walk reads the staged prefix)
// MISM: the 2 * (P.mism_hist + 2) words of the mismatch histogram
// INTERIOR: the 17 words [table | reads] of the interior table
// COMP: the 20 * P.composition words [c5 | c3] of the composition table
// SCORE: the 4 * P.score_half words of the score histogram (whole records are staged, as under -Q).  The weight table stays in
// global memory (beside the staging buffer it does not in general leave room for two workgroups per CU).
template <bool DO_PSS, bool DO_KMER, bool LDS_KMER, bool LATER_PASS = false, bool MASKQ = false, bool REGIONS = false, TallyArm ARM = ARM_NONE>
__global__ void __launch_bounds__(TILED_THREADS) tally_tiled(const TallyParams P) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    __shared__ __attribute__((aligned(16))) uint8_t sheet[TILED_MAX_T * 64u];
    __shared__ uint32_t table[TABLE_WORDS];
    __shared__ uint32_t toffs[2u * (TILED_MAX_T + 4u)];
    __shared__ uint32_t lds_kmer[LDS_KMER ? 2u * (1u << (2 * KMER_LDS_MAX_K)) : 1u];
    __shared__ int32_t lds_delta[ST_USED];
    __shared__ uint4 refs_lds[REF_LDS_ENTRIES + 1];
    // the kernel's single argument, as it lies in the kernarg segment (for the out-of-line path)
    const TallyParams *kernarg = (const TallyParams *)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr bool BEHIND = ARM == ARM_HIST || ARM == ARM_MISM || ARM == ARM_INTERIOR || ARM == ARM_COMP || ARM == ARM_SCORE;
    uint32_t *hist_lds = BEHIND ? (uint32_t *)(stage + tiled_lds_bytes(P.reads_per_tile, P.prefix_pieces)) : nullptr;
    if constexpr (ARM == ARM_SITE) {
        __shared__ uint32_t site_lds[SITE_WORDS];
        tally_tiled_body<DO_PSS, DO_KMER, LDS_KMER, LATER_PASS, PLANES_NONE, MASKQ, REGIONS, ARM>(P, kernarg, stage, sheet, table, toffs, lds_kmer, lds_delta,
                                                                                                  refs_lds, nullptr, nullptr, hist_lds, site_lds);
    } else if constexpr (ARM == ARM_END) {
        uint32_t *end_lds = (uint32_t *)(stage + tiled_lds_bytes(P.reads_per_tile, P.prefix_pieces));
        tally_tiled_body<DO_PSS, DO_KMER, LDS_KMER, LATER_PASS, PLANES_NONE, MASKQ, REGIONS, ARM>(P, kernarg, stage, sheet, table, toffs, lds_kmer, lds_delta,
                                                                                                  refs_lds, nullptr, nullptr, hist_lds, nullptr, end_lds);
    } else
    tally_tiled_body<DO_PSS, DO_KMER, LDS_KMER, LATER_PASS, PLANES_NONE, MASKQ, REGIONS, ARM>(P, kernarg, stage, sheet, table, toffs, lds_kmer, lds_delta,
                                                                                              refs_lds, nullptr, nullptr, hist_lds);
}

// ---------------------------------------------------------------------------------------
// -G / -S: one set of substitution tables per read group or per fragment-length bin, in one pass
// over the records
// ---------------------------------------------------------------------------------------
// The plane kernels take their PlaneParams as a second argument; it sits in the kernarg segment
// right behind TallyParams (HIP lays kernel arguments out in order at their natural alignment).
constexpr size_t PLANE_KERNARG_OFFSET = (sizeof(TallyParams) + alignof(PlaneParams) - 1) & ~(alignof(PlaneParams) - 1);

// tally_tiled with every record's counts in its plane (PLANES: by read group or by length bin).
// Dynamic LDS: the staging buffer, then (n_slots + 1) planes of 1024 words -- n_slots planes of
// this launch and the trash plane.  -G stages whole records (the RG tag sits behind QUAL); -S
// stages prefixes through QUAL[0] as tally_tiled does (whole records with -R only).  Substitution
// tables only.
template <PlaneSel PLANES, bool LATER_PASS, bool MASKQ = false, bool REGIONS = false>
__global__ void __launch_bounds__(TILED_THREADS) tally_tiled_planes(const TallyParams P, const PlaneParams G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    __shared__ __attribute__((aligned(16))) uint8_t sheet[TILED_MAX_T * 64u];
    __shared__ uint32_t toffs[2u * (TILED_MAX_T + 4u)];
    __shared__ uint32_t grp_lds[TILED_MAX_T];
    __shared__ uint32_t lds_kmer[1];
    __shared__ int32_t lds_delta[ST_USED];
    __shared__ uint4 refs_lds[REF_LDS_ENTRIES + 1];
    const TallyParams *kernarg = (const TallyParams *)__builtin_amdgcn_kernarg_segment_ptr();
    const PlaneParams *gk = (const PlaneParams *)((const uint8_t *)kernarg + PLANE_KERNARG_OFFSET);
    uint32_t *table = (uint32_t *)(stage + tiled_lds_bytes(P.reads_per_tile, P.prefix_pieces));
    if constexpr (PLANES == PLANES_EACH) {   // -A: n_slots resident planes + the trash plane, and who owns them
        __shared__ uint32_t each_lds[EACH_LDS_WORDS];
        tally_tiled_body<true, false, false, LATER_PASS, PLANES, MASKQ, REGIONS>(P, kernarg, stage, sheet, table, toffs, lds_kmer, lds_delta,
                                                                                 refs_lds, gk, grp_lds, nullptr, nullptr, nullptr, each_lds);
    } else
    tally_tiled_body<true, false, false, LATER_PASS, PLANES, MASKQ, REGIONS>(P, kernarg, stage, sheet, table, toffs, lds_kmer, lds_delta,
                                                                             refs_lds, gk, grp_lds);
}
// dynamic LDS a plane launch may take: the CU's 160 KiB less the kernel's static objects (~10.6 KiB) and some margin
constexpr uint32_t GROUPED_LDS_BUDGET = 148u * 1024u;
__host__ __device__ inline uint32_t tiled_grouped_lds_bytes(uint32_t T, uint32_t pieces, uint32_t n_slots) {
    return tiled_lds_bytes(T, pieces) + (n_slots + 1u) * GROUP_PLANE_WORDS * 4u;
}

// reduce_partials for tally_tiled_planes: slot layout [deltas 16 | n_slots planes]; plane slot s
// of the launch is plane plane0 + s of the counter block.  The status deltas (and the launch's
// record credit) belong to the launch of rows 0.. and planes 0..
__global__ void __launch_bounds__(256) reduce_partials_grouped(const TallyParams P, const PlaneParams G, uint32_t n_slots) {
    const uint32_t sw = G.scratch_words;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = gid % sw, g = gid / sw;
    if (g >= REDUCE_GROUPS) return;
    const uint32_t n_pos = (uint32_t)P.N + 2u;
    unsigned long long *dst = nullptr;
    bool is_delta = false;
    if (i < GROUP_SCRATCH_DELTA) {
        if (i < (uint32_t)ST_USED && P.row_base == 0u && G.plane0 == 0u) { dst = &P.counters[P.off_stats + i]; is_delta = true; }
    } else {
        const uint32_t w = (i - GROUP_SCRATCH_DELTA) & (GROUP_PLANE_WORDS - 1u), plane = G.plane0 + (i - GROUP_SCRATCH_DELTA) / GROUP_PLANE_WORDS;
        const uint32_t row = P.row_base + (w & 31u), ct = w >> 5, t = ct & 1u, cell = ct >> 1;
        const uint32_t base = plane ? G.off_groups + (plane - 1u) * G.plane_words : 0u;
        if (plane <= G.n_groups && row < n_pos) dst = &P.counters[base + (t ? P.off_rev : 0u) + row * 16u + cell];
    }
    if (!dst) return;
    long long sum = 0;
    const uint32_t *p = P.scratch + i;
#pragma unroll 8
    for (uint32_t b = g; b < n_slots; b += REDUCE_GROUPS) {
        const uint32_t v = p[(size_t)b * sw];
        sum += is_delta ? (long long)(int32_t)v : (long long)v;
    }
    if (is_delta && g == 0u && (i == ST_RECORDS || i == ST_PSS_OK)) sum += P.n_recs_dev ? *P.n_recs_dev : P.n_recs;
    if (sum) atomicAdd(dst, (unsigned long long)sum);
}

// tally_simple with every record's counts in its plane (global atomics; the cross-check of
// tally_tiled_planes).  Substitution tables only.
template <PlaneSel PLANES>
__global__ void __launch_bounds__(256) tally_simple_planes(const TallyParams P, const PlaneParams G) {
    __shared__ int32_t lds_delta[ST_USED];
    if (threadIdx.x < ST_USED) lds_delta[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < P.n_recs; r += stride) {
        const uint32_t o0 = P.offs[r], o1 = P.offs[r + 1];
        GlobalBytes src{P.recs + o0};
        const RecHdr h = decode_hdr(src, o1 - o0);
        const Plan pl = make_plan<true, false>(P, src, h);
        if (pl.pss_fwd || pl.pss_rev) {
            const uint32_t plane = record_plane<PLANES>(src, h, pl, G);
            if constexpr (PLANES == PLANES_EACH) {   // -A: plane = refID, every row at once
                uint32_t hit = 0u;
                tally_pss_record<true>(P, GlobalPlaneTable{P.counters + each_plane_base(G, plane), &hit, P.off_rev, 0u, 0xFFFFFFFFu}, src, h, pl);
                if (hit) P.counters[each_touched_base(G) + plane] = 1ull;
            } else {
            unsigned long long *base = P.counters + (plane ? G.off_groups + (plane - 1u) * G.plane_words : 0u);
            tally_pss_record<true>(P, GlobalTable{base, P.off_rev}, src, h, pl);
            }
        }
        book_events(true, false, record_events(true, false, pl, false), lds_delta);
    }
    __syncthreads();
    flush_events(true, false, P, lds_delta);
}

// ---------------------------------------------------------------------------------------
// fragkon -G / -S / -C: one [k5 | k3] pair of k-mer tables per plane, in one pass over the records
// ---------------------------------------------------------------------------------------
// tally_tiled's k-mer tally with every record's bins in its plane.  Dynamic LDS: the staging buffer, then (LDS_KMER,
// k <= KMER_LDS_MAX_K) n_slots + 1 histograms of 2 * 4^k words -- the planes of this launch and the trash slot; at
// k = 4 a plane is 2 KiB, so 64 length bins fit one launch.  Without LDS_KMER the bins go straight into the counter
// block with 64-bit atomics and one launch serves every plane.  No code sheet and no substitution table: the
// kernel's static LDS is the offsets, the deltas and the reference cache only.
template <PlaneSel PLANES, bool LDS_KMER, bool REGIONS = false>
__global__ void __launch_bounds__(TILED_THREADS) tally_tiled_kmer_planes(const TallyParams P, const PlaneParams G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t stage[];
    __shared__ uint32_t toffs[2u * (TILED_MAX_T + 4u)];
    __shared__ int32_t lds_delta[ST_USED];
    __shared__ uint4 refs_lds[REF_LDS_ENTRIES + 1];
    const TallyParams *kernarg = (const TallyParams *)__builtin_amdgcn_kernarg_segment_ptr();
    const PlaneParams *gk = (const PlaneParams *)((const uint8_t *)kernarg + PLANE_KERNARG_OFFSET);
    uint32_t *lds_kmer = (uint32_t *)(stage + tiled_lds_bytes(P.reads_per_tile, P.prefix_pieces));
    tally_tiled_body<false, true, LDS_KMER, false, PLANES, false, REGIONS>(P, kernarg, stage, nullptr, nullptr, toffs, lds_kmer, lds_delta,
                                                                           refs_lds, gk);
}
// dynamic LDS a k-mer plane launch may take: the CU's 160 KiB less the kernel's static objects (~2.1 KiB) and some margin
constexpr uint32_t KMER_PLANES_LDS_BUDGET = 156u * 1024u;
__host__ __device__ inline uint32_t tiled_kmer_planes_lds_bytes(uint32_t T, uint32_t pieces, uint32_t n_slots, int K, bool lds_kmer) {
    return tiled_lds_bytes(T, pieces) + (lds_kmer ? (n_slots + 1u) * 2u * (1u << (2 * K)) * 4u : 0u);
}

// reduce_partials for tally_tiled_kmer_planes: slot layout [deltas 16 | n_slots histograms of 2 * 4^k words]; histogram
// s of the launch is plane plane0 + s of the counter block, its words the plane's [k5 | k3] in order.  The status
// deltas (and the launch's record credit) belong to the launch of planes 0..
__global__ void __launch_bounds__(256) reduce_partials_kmer_planes(const TallyParams P, const PlaneParams G, uint32_t n_slots,
                                                                   uint32_t lds_kmer_on) {
    const uint32_t sw = G.scratch_words;
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t i = gid % sw, g = gid / sw;
    if (g >= REDUCE_GROUPS) return;
    unsigned long long *dst = nullptr;
    bool is_delta = false;
    if (i < GROUP_SCRATCH_DELTA) {
        if (i < (uint32_t)ST_USED && G.plane0 == 0u) { dst = &P.counters[P.off_stats + i]; is_delta = true; }
    } else if (lds_kmer_on) {
        const uint32_t kw = 2u * (1u << (2 * P.K));
        const uint32_t w = (i - GROUP_SCRATCH_DELTA) % kw, plane = G.plane0 + (i - GROUP_SCRATCH_DELTA) / kw;
        if (plane <= G.n_groups) dst = &P.counters[kmer_plane_base(P, G, plane) + w];
    }
    if (!dst) return;
    long long sum = 0;
    const uint32_t *p = P.scratch + i;
#pragma unroll 8
    for (uint32_t b = g; b < n_slots; b += REDUCE_GROUPS) {
        const uint32_t v = p[(size_t)b * sw];
        sum += is_delta ? (long long)(int32_t)v : (long long)v;
    }
    if (is_delta && g == 0u && (i == ST_RECORDS || i == ST_KMER_OK)) sum += P.n_recs_dev ? *P.n_recs_dev : P.n_recs;
    if (sum) atomicAdd(dst, (unsigned long long)sum);
}

// tally_simple's k-mer tally with every record's bins in its plane (global atomics; the cross-check of
// tally_tiled_kmer_planes)
template <PlaneSel PLANES>
__global__ void __launch_bounds__(256) tally_simple_kmer_planes(const TallyParams P, const PlaneParams G) {
    __shared__ int32_t lds_delta[ST_USED];
    if (threadIdx.x < ST_USED) lds_delta[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < P.n_recs; r += stride) {
        const uint32_t o0 = P.offs[r], o1 = P.offs[r + 1];
        GlobalBytes src{P.recs + o0};
        const RecHdr h = decode_hdr(src, o1 - o0);
        const Plan pl = make_plan<false, true>(P, src, h);
        bool kfail = false;
        if (pl.fk5 || pl.fk3) kfail = tally_kmer_record_plane<false>(P, G, pl, record_plane<PLANES, true>(src, h, pl, G), nullptr);
        book_events(false, true, record_events(false, true, pl, kfail), lds_delta);
    }
    __syncthreads();
    flush_events(false, true, P, lds_delta);
}

// genome-kmer-count (genome-kmer-count.c:69-79): every k-mer start of the device genome.  Each
// lane walks GKC_SPAN consecutive positions with a rolling 2-bit code; `run` = number of
// consecutive ACGT bases ending here, a window counts when run >= k.  Contig padding is stored
// as non-ACGT, so no window spans two contigs.  Bins: LDS histogram for k <= 6, else global.
constexpr uint32_t GKC_SPAN = 256;
template <bool LDS_BINS>
__global__ void __launch_bounds__(256) genome_kmer_kernel(const uint8_t *genome, uint64_t n, int K,
                                                          unsigned long long *bins) {
    __shared__ uint32_t lds_bins[LDS_BINS ? 4096 : 1];
    const uint32_t nb = 1u << (2 * K), mask = nb - 1u;
    if (LDS_BINS) {
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) lds_bins[i] = 0u;
        __syncthreads();
    }
    const uint64_t n_spans = (n + GKC_SPAN - 1) / GKC_SPAN;
    for (uint64_t sp = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sp < n_spans; sp += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p0 = sp * GKC_SPAN, p1 = min(n, p0 + GKC_SPAN);
        // warm-up: the K-1 bases before the span (their windows belong to the previous span)
        uint32_t code = 0u, run = 0u;
        for (uint64_t p = p0 >= (uint64_t)(K - 1) ? p0 - (uint64_t)(K - 1) : 0; p < p0; p++) {
            const uint32_t c = genome[p];
            run = c < 4u ? run + 1u : 0u;
            code = ((code << 2) | (c & 3u)) & mask;
        }
        for (uint64_t p = p0; p < p1; p += 4) {  // spans start 4-byte aligned (GKC_SPAN % 4 == 0)
            const uint32_t w = *(const uint32_t *)(genome + p);
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (p + b < p1) {
                    const uint32_t c = (w >> (8 * b)) & 0xFFu;
                    run = c < 4u ? run + 1u : 0u;
                    code = ((code << 2) | (c & 3u)) & mask;
                    if (run >= (uint32_t)K) {  // window [p+b-K+1, p+b] is all ACGT
                        if (LDS_BINS) atomicAdd(&lds_bins[code], 1u);
                        else atomicAdd(&bins[code], 1ull);
                    }
                }
            }
        }
    }
    if (LDS_BINS) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x)
            if (lds_bins[i]) atomicAdd(&bins[i], (unsigned long long)lds_bins[i]);
    }
}

// The same census for k <= 8 from the 4-bit packed genome, with the whole histogram (or half of
// it per pass at k = 8) in LDS:
//   - a lane walks GKC4_SPAN consecutive positions = 128 packed bytes with a rolling 2-bit code,
//     eight dwordx4 loads per span;
//   - bins are REPLICATED rep times (lane & (rep-1) picks the copy, copies of a bin sit in adjacent
//     words = different banks): the AAAA / TTTT / poly-N skew of a real genome would otherwise
//     serialise the lanes of a wave on a few words;
//   - bin_lo / n_bins select the slice of the 4^k bins this pass owns (k = 8: two passes of 32 Ki
//     bins = 128 KiB of LDS each); one u64 global atomic per non-empty bin per workgroup at the end.
constexpr uint32_t GKC4_SPAN = 256;
__global__ void __launch_bounds__(512) genome_kmer_packed_kernel(const uint32_t *g4, uint64_t n_pos, int K, uint32_t bin_lo,
                                                                 uint32_t n_bins, uint32_t rep_log2,
                                                                 unsigned long long *bins) {
    extern __shared__ uint32_t lds_hist[];
    const uint32_t rep = 1u << rep_log2;
    for (uint32_t i = threadIdx.x; i < (n_bins << rep_log2); i += blockDim.x) lds_hist[i] = 0u;
    __syncthreads();
    const uint32_t mask = (1u << (2 * K)) - 1u;
    const uint32_t copy = threadIdx.x & (rep - 1u);
    const uint64_t n_spans = (n_pos + GKC4_SPAN - 1) / GKC4_SPAN;
    for (uint64_t sp = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; sp < n_spans; sp += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p0 = sp * GKC4_SPAN;
        const uint4 *src = (const uint4 *)(g4 + p0 / 8);
        uint32_t code = 0u, run = 0u;
        if (p0) {  // warm-up: the K-1 <= 7 positions before the span are in the previous dword
            const uint32_t w = g4[p0 / 8 - 1];
#pragma unroll
            for (int b = 1; b < 8; b++) {
                const uint32_t c = (w >> (4 * b)) & 15u;
                run = c < 4u ? run + 1u : 0u;
                code = (code << 2) | (c & 3u);
            }
            run = min(run, (uint32_t)(K - 1));  // windows starting before the span belong to the previous one
        }
#pragma unroll 2
        for (int q = 0; q < (int)(GKC4_SPAN / 32); q++) {
            if (p0 + 32ull * q >= n_pos) break;
            const uint4 v = src[q];
            const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int d = 0; d < 4; d++) {
#pragma unroll
                for (int b = 0; b < 8; b++) {
                    const uint32_t c = (w4[d] >> (4 * b)) & 15u;
                    run = c < 4u ? run + 1u : 0u;
                    code = ((code << 2) | (c & 3u)) & mask;
                    const uint32_t slot = code - bin_lo;
                    if (run >= (uint32_t)K && slot < n_bins && p0 + 32ull * q + 8u * d + b < n_pos)
                        atomicAdd(&lds_hist[(slot << rep_log2) + copy], 1u);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_bins; i += blockDim.x) {
        uint32_t sum = 0u;
        for (uint32_t r = 0; r < rep; r++) sum += lds_hist[(i << rep_log2) + r];
        if (sum) atomicAdd(&bins[bin_lo + i], (unsigned long long)sum);
    }
}

// Upload-time genome transform: toupper() fold (init_genome stores upper case,
// fasta-genome-io.c:127; process_aln folds again, pss-bam.c:424) followed by the
// A/C/G/T <-> 0..3 byte swap of record_decode.h.  16 bytes per lane per step.
// a small table from page-locked host memory into device memory (engine.hip: the reference table)
__global__ void copy_table_kernel(uint4 *dst, const uint4 *src, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

__global__ void encode_genome_kernel(uint8_t *p, uint64_t n16) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint4 *q = (uint4 *)p;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        uint4 v = q[i];
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t o = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                uint32_t c = (w[k] >> (8 * b)) & 0xFFu;
                if (c >= 'a' && c <= 'z') c -= 32u;
                o |= enc_byte(c) << (8 * b);
            }
            w[k] = o;
        }
        q[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// The tiled kernel's 4-bit image of the stored genome (record_decode.h, TallyParams::genome4):
// one output dword = 8 consecutive positions, little-endian in nibbles.
struct CtxSets { uint32_t up[8], down[8]; };
__global__ void pack_genome4_kernel(const uint8_t *g, uint32_t *out, uint64_t n_out, CtxSets sets) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint2 *src = (const uint2 *)g;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += stride) {
        const uint2 v = src[i];
        uint32_t o = 0u;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint32_t c = ((b < 4 ? v.x : v.y) >> (8 * (b & 3))) & 0xFFu;
            const uint32_t nib = c < 4u ? c : 4u + (in_set(sets.up, c) ? 1u : 0u) + (in_set(sets.down, c) ? 2u : 0u);
            o |= nib << (4 * b);
        }
        out[i] = o;
    }
}

}  // namespace pssbam

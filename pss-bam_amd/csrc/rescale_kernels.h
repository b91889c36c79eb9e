// pss-bam_amd/csrc/rescale_kernels.h -- the quality rescale of kept BAM records (the soft alternative to the end mask of
// end_mask_kernels.h), per record: the QUAL byte of every read base that the substitution tally adds to cell (read T, reference C) of
// one of the first D rows of the forward table -- or to cell (A, G) (DS) or (T, C) (SS) of one of the first D rows of the reverse
// table -- is replaced by table[end][row][q] in a copy of the record.  DESIGN 4.2y.
//
//   pssbam_rescale_record     one record: the header fields of the input record, the bounds rule, the two walks.  Plain C that also
//                             compiles as HIP device code (no kernel launches it yet: DESIGN 4.2y says why); host/hostcheck_main.c
//                             and tools/rescale_emulate.cpp run it.  Which tables the record was added to, and where it lies on
//                             the reference, is the caller's to say.
//   pssbam_rescale_host_plan  the tally's decision under pss-bam's defaults, for those two host drivers.
//
// A candidate is stated in the coordinates of tally_end (tally_kernels.h): the forward table is fed from the alignment's left end
// on a forward and from its right end, complemented, on a reverse read; the reverse table the other way round.  Cell c of a
// complemented walk is cell 15 - c of the stored bases, so the stored pair that is looked for is (T, C) or (A, G), by end and strand.
// The stored SEQ nibble is tested first; the genome byte is loaded only for the quarter or so of the positions that pass.
//
// Writes are single QUAL bytes of the record's own copy (the ownership argument of end_mask_kernels.h, unchanged).  The walk reads
// SEQ and QUAL of the INPUT record, never of the copy: -Q judges the original quality, and a byte that is a candidate of both
// walks (SS, reads shorter than 2 D) gets the smaller of the two entries of its original value, whichever walk comes first.
#ifndef PSSBAM_RESCALE_KERNELS_H
#define PSSBAM_RESCALE_KERNELS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define PSSBAM_RS_FN __host__ __device__ __forceinline__
#else
#define PSSBAM_RS_FN static inline
#endif

#define PSSBAM_RS_OFF 0
#define PSSBAM_RS_DS 1
#define PSSBAM_RS_SS 2
#define PSSBAM_RS_MAX_ROWS 64u
#define PSSBAM_RS_QUALS 94u   /* table columns: q = 0..93 */

/* a little-endian dword at any alignment */
PSSBAM_RS_FN uint32_t pssbam_rs_u32(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

/* counts[((end * rows) + row) * 2 + {0: candidates, 1: lowered}]; in device code the words may be shared by a workgroup (LDS) */
PSSBAM_RS_FN void pssbam_rs_count(uint32_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)__hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    (*p)++;
#endif
}

/* One record.  in: the input record of `len` bytes (block_size first); out: its copy in the output, the only thing written.
 * G: the stored bytes of the record's contig (A C G T = 0 1 2 3), G[p] = contig position p; s, L: the alignment's start and the
 * length the tally gave the read (|TLEN| for a paired one); rev: FLAG 0x10; in_fwd / in_rev: the tally added the read to the
 * forward / the reverse table.  The caller vouches for 0 <= s and s + L <= the contig's length (a tallied read has two bases more on
 * either side) and for L >= D.  mode: PSSBAM_RS_DS or _SS; the first D <= rows rows of each end are walked; min_bq: the tally's -Q (0: none); table: [2][rows][94].
 * A record whose fields do not fit inside it is left as it is and counts nothing. */
PSSBAM_RS_FN void pssbam_rescale_record(const uint8_t *in, uint8_t *out, uint32_t len, const uint8_t *G, int64_t s, uint32_t L, uint32_t rev,
                                        uint32_t in_fwd, uint32_t in_rev, uint32_t mode, uint32_t D, uint32_t rows, uint32_t min_bq, const uint8_t *table,
                                        uint32_t *counts)
{
    if (len < 36u || (mode != PSSBAM_RS_DS && mode != PSSBAM_RS_SS) || D == 0u || D > rows || rows > PSSBAM_RS_MAX_ROWS || L < D) return;
    const uint32_t block_size = pssbam_rs_u32(in), w12 = pssbam_rs_u32(in + 12), w16 = pssbam_rs_u32(in + 16), l = pssbam_rs_u32(in + 20);
    const uint32_t l_read_name = w12 & 0xFFu, n_cigar_op = w16 & 0xFFFFu;
    const uint64_t seq_at = 36ull + l_read_name + 4ull * n_cigar_op, qual_at = seq_at + ((uint64_t)l + 1ull) / 2ull;
    uint64_t have = 4ull + block_size;
    if (have > len) have = len;
    if (l == 0u || qual_at + l > have) return;
    const uint8_t *seq = in + seq_at, *qual = in + qual_at;
    uint8_t *qout = out + qual_at;
    const uint32_t absent = qual[0] == 0xFFu;   /* qualities absent: candidates are counted, nothing is written */
    for (uint32_t end = 0; end < 2u; end++) {
        if (!(end ? in_rev : in_fwd)) continue;
        /* tally_end's `left`: the forward table takes the left end of a forward read, the reverse table that of a reverse read */
        const uint32_t left = end ? rev : !rev;
        /* the cell in table coordinates is (T, C) = 13, or (A, G) = 2 at the 3' end of a double-stranded library; a reverse read's
         * stored bases are the complement: (A, G) for 13, (T, C) for 2 */
        const uint32_t want_tc = (end == 0u || mode == PSSBAM_RS_SS) ? !rev : rev;
        const uint32_t code = want_tc ? 8u : 1u, ref = want_tc ? 1u : 2u;   /* stored SEQ code T / A, stored genome byte C / G */
        const uint8_t *row = table + (size_t)end * rows * PSSBAM_RS_QUALS;
        uint32_t *cnt = counts + (size_t)end * rows * 2u;
        for (uint32_t i = 0; i < D; i++) {
            const uint32_t ri = left ? i : L - 1u - i;
            if (ri >= l) continue;   /* (a mate whose SEQ is shorter than |TLEN|: the tally reads no base there) */
            const uint32_t by = seq[ri >> 1], nib = (ri & 1u) ? (by & 15u) : (by >> 4);
            if (nib != code) continue;
            const uint32_t q = qual[ri];
            if (q < min_bq) continue;   /* -Q: the base was not tallied (absent qualities are 0xFF: never below) */
            if (G[s + (int64_t)ri] != ref) continue;
            pssbam_rs_count(cnt + 2u * i);
            if (absent || q >= PSSBAM_RS_QUALS) continue;
            const uint32_t nq = row[(size_t)i * PSSBAM_RS_QUALS + q];
            if (nq >= q) continue;
            pssbam_rs_count(cnt + 2u * i + 1u);
            if (nq < qout[ri]) qout[ri] = (uint8_t)nq;   /* (its own byte: what the other walk may have left there) */
        }
    }
}

#if !defined(__HIPCC__)
/* The tally's decision for the host drivers (hostcheck -k, tools/rescale_emulate.cpp), which have no engine: make_plan of
 * csrc/record_decode.h under pss-bam's defaults but -r and -q -- <L>M records, no read-group, length, context-set (-U / -D other than
 * ACGT), region, mismatch or score filter.  contigs[refID] / contig_len[refID]: the stored bytes of the BAM's references (NULL: the
 * genome lacks it).  Returns non-zero when the record is added to a main table, with the arguments of pssbam_rescale_record. */
static inline int pssbam_rescale_host_plan(const uint8_t *rec, uint32_t len, const uint8_t *const *contigs, const uint32_t *contig_len, int32_t n_ref,
                                           uint32_t region_len, uint32_t min_mq, const uint8_t **G, int64_t *s, uint32_t *L, uint32_t *rev, uint32_t *in_fwd,
                                           uint32_t *in_rev)
{
    if (len < 36u) return 0;
    const uint32_t block_size = pssbam_rs_u32(rec), w12 = pssbam_rs_u32(rec + 12), w16 = pssbam_rs_u32(rec + 16), l = pssbam_rs_u32(rec + 20);
    const int32_t ref_id = (int32_t)pssbam_rs_u32(rec + 4), pos = (int32_t)pssbam_rs_u32(rec + 8), tlen = (int32_t)pssbam_rs_u32(rec + 32);
    const uint32_t l_read_name = w12 & 0xFFu, mapq = (w12 >> 8) & 0xFFu, n_cigar_op = w16 & 0xFFFFu, flag = w16 >> 16;
    const uint64_t cig_at = 36ull + l_read_name, seq_at = cig_at + 4ull * n_cigar_op, qual_at = seq_at + ((uint64_t)l + 1ull) / 2ull;
    if (4ull + block_size != len || qual_at + l > len) return 0;
    const uint32_t l_text = l ? l : 1u, q0 = l ? rec[qual_at] : 0xFFu;
    if (q0 == 0xFFu && l_text != 1u) return 0;                                  /* SEQ and QUAL of different lengths as text */
    if (ref_id < 0 || ref_id >= n_ref || !contigs[ref_id]) return 0;
    const uint32_t glen = contig_len[ref_id], paired = flag & 1u;
    if (n_cigar_op != 1u || (flag & (0x4u | 0x100u | 0x200u | 0x400u | 0x800u)) || pos < 0) return 0;
    const uint32_t c0 = pssbam_rs_u32(rec + cig_at);
    const uint32_t len_t = paired ? (uint32_t)(tlen < 0 ? -(int64_t)tlen : (int64_t)tlen) : l_text;
    if ((c0 & 15u) != 0u || (c0 >> 4) != len_t) return 0;
    if (glen < 4u || len_t > glen - 4u || pos < 2 || (uint32_t)pos - 2u > glen - 4u - len_t) return 0;
    if (mapq < min_mq || len_t < region_len) return 0;
    if (paired && ((flag & 0xAu) != 0x2u || !(flag & 0xC0u))) return 0;       /* proper pair, mate mapped, a mate number */
    const uint8_t *g = contigs[ref_id];
    const uint32_t is_rev = (flag >> 4) & 1u, l1 = g[pos - 1], r1 = g[(int64_t)pos + len_t];
    const uint32_t up_ok = (is_rev ? r1 : l1) < 4u, dn_ok = (is_rev ? l1 : r1) < 4u;   /* -U / -D ACGT: the complement of a base is a base */
    const uint32_t r1st = (flag & 0x40u) != 0u, r2nd = (flag & 0x80u) != 0u;
    *in_fwd = paired ? (r1st && up_ok) : (up_ok && dn_ok);
    *in_rev = paired ? (!(r1st && up_ok) && r2nd && dn_ok) : (up_ok && dn_ok);
    *G = g;
    *s = pos;
    *L = len_t;
    *rev = is_rev;
    return *in_fwd || *in_rev;
}
#endif

#endif

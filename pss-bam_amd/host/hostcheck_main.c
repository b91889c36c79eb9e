/*
 * pss-bam_amd/host/hostcheck_main.c -- `hostcheck [-f genome.fa] [-a alignments [-w out.bam [-z level] [-t threads]]]`: drives every
 * multi-threaded piece of the host library without a GPU and prints a digest of what came out:
 * the FASTA loader (block + parallel parser), the three-stage BGZF/BAM reader and the threaded
 * SAM-text reader; with -w also the BAM writer (bam_writer.h), which then receives every batch of a
 * BAM input as it comes from the reader; with -w and -b the record stream is cut into BGZF payloads of 0xFF00 bytes at fixed
 * offsets here (records cross blocks), every payload is deflated with zlib, and the finished blocks reach the writer through
 * bam_writer_append_blocks in uneven pieces -- the path of pss-bam -O ... -Z without a GPU (-x trunc / -x chain damage the last
 * piece: the call must fail and leave no file); with -w and -K <all|ds|ss>,<n5>[,<n3>] every record passes through the end mask
 * of pss-bam -K on its way to the writer -- the per-record function the device kernel runs (csrc/end_mask_kernels.h), compiled
 * for the host; with -w and -k <ds|ss>,<rates file>[,<baseline>] (and -f, -r <region_len>, -M <min mapq>) every record that pss-bam
 * -r -q would add to a table passes through the quality rescale first -- the table builder (rescale.h) and the
 * per-record function of the device kernel (csrc/rescale_kernels.h), the plan restated for the host there -- and the candidate counts
 * are printed; with -s <sites.txt> the sites-file reader of pss-bam -a (alleles.h) runs over the file and, with -S <prefix>, its
 * report writer over made-up counts for the sites read (a refused file is exit 1 with the reader's message).  It exists for the
 * sanitizer builds (`make sanitize`: ThreadSanitizer and
 * AddressSanitizer + UBSan; tests/test_sanitizers.py) -- the digests of the instrumented
 * binaries must equal the plain build's, and the sanitizers must stay silent.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "alleles.h"
#include "bam_reader.h"
#include "bam_writer.h"
#include "end_mask.h"
#include "end_mask_kernels.h"
#include "fasta-genome-io.h"
#include "rescale.h"
#include "rescale_kernels.h"
#include "sam_reader.h"

#include <zlib.h>

static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

/* -b: the blocks made so far and the tail of the stream that has not filled a payload yet */
struct reblock {
    uint8_t *pend, *blk;
    size_t n_pend, cap_pend, n_blk, cap_blk, n_blocks, piece;
    int level;
};

static int reblock_one(struct reblock *r, const uint8_t *src, uint32_t len)
{
    if (r->cap_blk - r->n_blk < 0x10000u) {
        r->cap_blk = r->cap_blk * 2 + 0x20000u;
        r->blk = (uint8_t *)realloc(r->blk, r->cap_blk);
        if (!r->blk) return -1;
    }
    uint8_t *dst = r->blk + r->n_blk;
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (deflateInit2(&zs, r->level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return -1;
    zs.next_in = (Bytef *)src;
    zs.avail_in = len;
    zs.next_out = dst + 18;
    zs.avail_out = 0x10000u - 26u;
    const int zrc = deflate(&zs, Z_FINISH);
    const uint32_t total = 18u + (uint32_t)zs.total_out + 8u;
    deflateEnd(&zs);
    if (zrc != Z_STREAM_END) return -1;
    static const uint8_t head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
    memcpy(dst, head, 16);
    dst[16] = (uint8_t)((total - 1u) & 0xffu);
    dst[17] = (uint8_t)((total - 1u) >> 8);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len);
    for (int i = 0; i < 4; i++) {
        dst[total - 8 + i] = (uint8_t)(crc >> (8 * i));
        dst[total - 4 + i] = (uint8_t)(len >> (8 * i));
    }
    r->n_blk += total;
    r->n_blocks++;
    return 0;
}

/* hands the blocks made so far to the writer once there are as many as the next piece takes: 1, 3, 7, 2, 5 blocks in turn */
static int reblock_hand_over(struct reblock *r, bam_writer *wr, int last, const char *damage)
{
    static const size_t pieces[5] = {1, 3, 7, 2, 5};
    if (!last && r->n_blocks < pieces[r->piece % 5]) return 0;
    size_t n = r->n_blk;
    if (last && damage && n) {
        if (!strcmp(damage, "trunc")) n -= 5;
        else r->blk[16] ^= 0x10;   /* chain: the first BSIZE of the piece no longer leads to a header */
    }
    const int rc = bam_writer_append_blocks(wr, r->blk, n);
    r->n_blk = r->n_blocks = 0;
    r->piece++;
    return rc;
}

static int reblock_add(struct reblock *r, bam_writer *wr, const uint8_t *p, size_t n)
{
    if (r->cap_pend - r->n_pend < n) {
        r->cap_pend = (r->n_pend + n) * 2;
        r->pend = (uint8_t *)realloc(r->pend, r->cap_pend);
        if (!r->pend) return -1;
    }
    memcpy(r->pend + r->n_pend, p, n);
    r->n_pend += n;
    size_t o = 0;
    for (; r->n_pend - o >= BAM_WRITER_BLOCK_MAX; o += BAM_WRITER_BLOCK_MAX) {
        if (reblock_one(r, r->pend + o, BAM_WRITER_BLOCK_MAX)) return -1;
        if (reblock_hand_over(r, wr, 0, NULL)) return -1;
    }
    memmove(r->pend, r->pend + o, r->n_pend - o);
    r->n_pend -= o;
    return 0;
}

int main(int argc, char **argv)
{
    const char *fa = NULL, *aln = NULL, *out = NULL, *sites_fn = NULL, *sites_out = NULL;
    int level = 1, wthreads = 0, blocks = 0;
    const char *damage = NULL, *mask_arg = NULL;
    int mask_mode = PSSBAM_EM_OFF;
    uint32_t mask_n5 = 0, mask_n3 = 0;
    uint8_t *masked = NULL;   /* -K: the batch on its way to the writer */
    size_t masked_cap = 0;
    const char *rescale_arg = NULL;   /* -k, with -r and -M */
    static pss_rescale rescale;
    uint32_t region_len = 15, min_mq = 0;
    static uint32_t rs_counts[4 * PSS_RESCALE_MAX_ROWS];
    static uint64_t rs_total[4 * PSS_RESCALE_MAX_ROWS];
    int quick = 0; /* -q: no digest, just drain the reader and report its inflate seconds (throughput probe) */
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "-q")) { quick = 1; continue; }
        if (!strcmp(argv[i], "-f") && i + 1 < argc) fa = argv[++i];
        else if (!strcmp(argv[i], "-a") && i + 1 < argc) aln = argv[++i];
        else if (!strcmp(argv[i], "-w") && i + 1 < argc) out = argv[++i];
        else if (!strcmp(argv[i], "-z") && i + 1 < argc) level = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-t") && i + 1 < argc) wthreads = atoi(argv[++i]);
        else if (!strcmp(argv[i], "-b")) blocks = 1;
        else if (!strcmp(argv[i], "-x") && i + 1 < argc) damage = argv[++i];
        else if (!strcmp(argv[i], "-K") && i + 1 < argc) mask_arg = argv[++i];
        else if (!strcmp(argv[i], "-k") && i + 1 < argc) rescale_arg = argv[++i];
        else if (!strcmp(argv[i], "-r") && i + 1 < argc) region_len = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-M") && i + 1 < argc) min_mq = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "-s") && i + 1 < argc) sites_fn = argv[++i];
        else if (!strcmp(argv[i], "-S") && i + 1 < argc) sites_out = argv[++i];
    }
    if (mask_arg) {
        char err[200];
        if (pss_parse_end_mask(mask_arg, &mask_mode, &mask_n5, &mask_n3, err, sizeof err)) { fprintf(stderr, "hostcheck: %s\n", err); return 1; }
        if (!out) { fprintf(stderr, "hostcheck: -K masks what -w writes\n"); return 1; }
    }
    if (rescale_arg) {
        char err[700];
        if (pss_parse_rescale(rescale_arg, &rescale, NULL, err, sizeof err)) { fprintf(stderr, "hostcheck: %s\n", err); return 1; }
        if (!out || !fa) { fprintf(stderr, "hostcheck: -k rescales what -w writes, against the genome of -f\n"); return 1; }
    }
    if (!fa && !aln && !sites_fn) {
        fprintf(stderr, "usage: hostcheck [-f genome.fa[.gz]] [-a file.bam|file.sam[.gz] [-w out.bam [-z level] [-t threads] [-b [-x trunc|chain]] [-K mode,n5[,n3]] [-k mode,rates[,baseline] [-r region_len] [-M min_mapq]]]] [-s sites.txt [-S prefix]]\n");
        return 2;
    }
    if (sites_fn) {   /* pss-bam -a: the reader, and the writer over counts made up from the site's number */
        char err[600];
        pss_sites st;
        if (pss_read_sites(sites_fn, &st, err, sizeof err)) { fprintf(stderr, "hostcheck: %s\n", err); return 1; }
        uint64_t h = 1469598103934665603ull;
        for (int32_t k = 0; k < st.n_names; k++) h = fnv(h, st.names[k], strlen(st.names[k]) + 1);
        h = fnv(h, st.name_of, (size_t)st.n * sizeof *st.name_of);
        h = fnv(h, st.pos0, (size_t)st.n * sizeof *st.pos0);
        printf("sites names=%d sites=%lld digest=%016llx\n", (int)st.n_names, (long long)st.n, (unsigned long long)h);
        if (sites_out) {   /* arrays of exactly the sites' size: a stray read is one past a heap block */
            const size_t n = (size_t)st.n;
            uint8_t *base = (uint8_t *)malloc(n);
            uint32_t *counts = (uint32_t *)malloc(n * 10 * sizeof *counts);
            if (!base || !counts) { fprintf(stderr, "hostcheck: out of memory\n"); return 1; }
            uint64_t totals[4] = {n, n, 0, 0};
            for (size_t i = 0; i < n; i++) {
                base[i] = (uint8_t)"ACGTN"[i % 5];
                uint64_t sum = 0;
                for (size_t w = 0; w < 10; w++) sum += counts[10 * i + w] = (uint32_t)((i * 7 + w * 3) % 5 == 0 ? i + w : 0);
                totals[2] += sum != 0;
                totals[3] += sum;
            }
            const int32_t first = st.name_of[0];
            st.name_of[0] = st.n_names;   /* a reference the list lacks: refused, and no file is left */
            if (!pss_write_alleles("genome.fa", "reads.bam", sites_fn, 2, sites_out, st.n_names, (const char *const *)st.names, (uint64_t)n, st.name_of, st.pos0, base,
                                   counts, totals)) {
                fprintf(stderr, "hostcheck: the writer took a site on a reference it does not have\n");
                return 1;
            }
            st.name_of[0] = first;
            if (pss_write_alleles("genome.fa", "reads.bam", sites_fn, 2, sites_out, st.n_names, (const char *const *)st.names, (uint64_t)n, st.name_of, st.pos0, base,
                                  counts, totals))
                return 1;
            free(base);
            free(counts);
        }
        pss_free_sites(&st);
    }
    Genome *genome = NULL;   /* -k: kept for the records */
    if (fa) {
        Genome *g = init_genome(fa);
        if (!g) { fprintf(stderr, "hostcheck: cannot load %s\n", fa); return 1; }
        uint64_t h = 1469598103934665603ull, bases = 0;
        for (size_t i = 0; i < g->n_seqs; i++) {
            h = fnv(h, g->seqs[i]->id, strlen(g->seqs[i]->id) + 1);
            h = fnv(h, g->seqs[i]->seq, g->seqs[i]->len);
            bases += g->seqs[i]->len;
        }
        printf("genome seqs=%zu bases=%llu digest=%016llx\n", (size_t)g->n_seqs, (unsigned long long)bases, (unsigned long long)h);
        if (rescale_arg) genome = g;
        else destroy_genome(g);
    }
    if (aln) {
        char err[512];
        const int is_bam = file_is_bam(aln);
        if (is_bam < 0) { fprintf(stderr, "hostcheck: cannot open %s\n", aln); return 1; }
        bam_reader *rd = is_bam ? bam_reader_open(aln, 0, 0, err, sizeof err) : NULL;
        sam_reader *sd = is_bam ? NULL : sam_reader_open(aln, 0, err, sizeof err);
        if (!rd && !sd) { fprintf(stderr, "hostcheck: %s\n", err); return 1; }
        bam_writer *wr = NULL;
        if (out) {   /* the round trip through the writer: header from the reader's, every batch appended */
            if (!rd) { fprintf(stderr, "hostcheck: -w takes a BAM input\n"); return 1; }
            wr = bam_writer_open(out, bam_reader_header(rd), level, wthreads);
            if (!wr) { fprintf(stderr, "hostcheck: %s\n", bam_writer_open_error()); return 1; }
        }
        /* -k: the BAM's references in the genome's stored form (A C G T = 0 1 2 3 after the upper-case fold, everything else itself) */
        uint8_t **contigs = NULL;
        uint32_t *contig_len = NULL;
        const int32_t n_contigs = rescale_arg && rd ? bam_reader_header(rd)->n_ref : 0;
        const uint32_t rs_d = rescale.rows < region_len ? rescale.rows : region_len;
        if (rescale_arg) {
            contigs = (uint8_t **)calloc((size_t)n_contigs + 1, sizeof *contigs);
            contig_len = (uint32_t *)calloc((size_t)n_contigs + 1, sizeof *contig_len);
            if (!contigs || !contig_len) { fprintf(stderr, "hostcheck: out of memory\n"); return 1; }
            for (int32_t k = 0; k < n_contigs; k++) {
                const Seq *sq = find_seq(genome, bam_reader_header(rd)->ref_name[k]);
                if (!sq || sq->len > 0xFFFFFFFFu) continue;
                contigs[k] = (uint8_t *)malloc(sq->len ? sq->len : 1);
                if (!contigs[k]) { fprintf(stderr, "hostcheck: out of memory\n"); return 1; }
                contig_len[k] = (uint32_t)sq->len;
                for (size_t j = 0; j < sq->len; j++) {
                    const int c = sq->seq[j] >= 'a' && sq->seq[j] <= 'z' ? sq->seq[j] - 32 : (unsigned char)sq->seq[j];
                    contigs[k][j] = (uint8_t)(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : c);
                }
            }
        }
        struct reblock rb;
        memset(&rb, 0, sizeof rb);
        rb.level = level;
        uint64_t h = 1469598103934665603ull, recs = 0, bytes = 0, batches = 0;
        for (;;) {
            const uint8_t *p;
            const uint32_t *offs;
            size_t nbytes;
            const int64_t n = rd ? bam_reader_next(rd, &p, &offs, &nbytes) : sam_reader_next(sd, &p, &offs, &nbytes);
            if (n < 0) { fprintf(stderr, "hostcheck: %s\n", rd ? bam_reader_error(rd) : sam_reader_error(sd)); return 1; }
            if (n == 0) break;
            if (offs[0] != 0 || offs[n] != nbytes) { fprintf(stderr, "hostcheck: offset index does not cover the batch\n"); return 1; }
            for (int64_t i = 0; i < n && !quick; i++) {   /* every record is exactly its block_size */
                uint32_t bs;
                memcpy(&bs, p + offs[i], 4);
                if (offs[i + 1] - offs[i] != 4u + bs) { fprintf(stderr, "hostcheck: record %lld mis-indexed\n", (long long)(recs + i)); return 1; }
            }
            if (!quick) h = fnv(h, p, nbytes);
            if (wr && rescale_arg) {   /* -k in front of -K, as on the device: a buffer of exactly the batch's size here too */
                if (masked_cap != nbytes) {
                    free(masked);
                    masked = (uint8_t *)malloc(nbytes ? nbytes : 1);
                    masked_cap = nbytes;
                    if (!masked) { fprintf(stderr, "hostcheck: out of memory\n"); return 1; }
                }
                memcpy(masked, p, nbytes);
                memset(rs_counts, 0, sizeof rs_counts);
                for (int64_t i = 0; i < n && rs_d; i++) {
                    const uint8_t *G;
                    int64_t s;
                    uint32_t L, rev, in_fwd, in_rev;
                    const uint32_t len = offs[i + 1] - offs[i];
                    if (!pssbam_rescale_host_plan(p + offs[i], len, (const uint8_t *const *)contigs, contig_len, n_contigs, region_len, min_mq, &G, &s, &L, &rev, &in_fwd, &in_rev))
                        continue;
                    pssbam_rescale_record(p + offs[i], masked + offs[i], len, G, s, L, rev, in_fwd, in_rev, (uint32_t)rescale.mode, rs_d, rescale.rows, 0u,
                                          rescale.table, rs_counts);
                }
                for (size_t k = 0; k < 4 * (size_t)rescale.rows; k++) rs_total[k] += rs_counts[k];
                if (mask_mode != PSSBAM_EM_OFF)
                    for (int64_t i = 0; i < n; i++) pssbam_end_mask_record(masked + offs[i], offs[i + 1] - offs[i], (uint32_t)mask_mode, mask_n5, mask_n3);
                p = masked;
            } else
            if (wr && mask_mode != PSSBAM_EM_OFF) {   /* a buffer of exactly the batch's size: a stray write is one past a heap block */
                if (masked_cap != nbytes) {
                    free(masked);
                    masked = (uint8_t *)malloc(nbytes ? nbytes : 1);
                    masked_cap = nbytes;
                    if (!masked) { fprintf(stderr, "hostcheck: out of memory\n"); return 1; }
                }
                memcpy(masked, p, nbytes);
                for (int64_t i = 0; i < n; i++) pssbam_end_mask_record(masked + offs[i], offs[i + 1] - offs[i], (uint32_t)mask_mode, mask_n5, mask_n3);
                p = masked;
            }
            if (wr && (blocks ? reblock_add(&rb, wr, p, nbytes) : bam_writer_append(wr, p, nbytes))) {
                fprintf(stderr, "hostcheck: %s\n", bam_writer_error(wr));
                bam_writer_abort(wr);
                return 1;
            }
            recs += (uint64_t)n;
            bytes += nbytes;
            batches++;
        }
        if (wr && blocks) {   /* the short last payload, and whatever has not been handed over */
            if ((rb.n_pend && reblock_one(&rb, rb.pend, (uint32_t)rb.n_pend)) || reblock_hand_over(&rb, wr, 1, damage)) {
                fprintf(stderr, "hostcheck: %s\n", bam_writer_error(wr));
                bam_writer_abort(wr);
                free(rb.pend);
                free(rb.blk);
                bam_reader_close(rd);
                return 1;
            }
            free(rb.pend);
            free(rb.blk);
        }
        free(masked);
        for (int32_t k = 0; k < n_contigs; k++) free(contigs[k]);
        free(contigs);
        free(contig_len);
        if (rescale_arg)
            for (uint32_t k = 0; k < 2 * rs_d; k++)
                printf("rescale end=%d row=%u candidates=%llu lowered=%llu\n", k < rs_d ? 5 : 3, k % rs_d, (unsigned long long)rs_total[2 * ((k / rs_d) * rescale.rows + k % rs_d)],
                       (unsigned long long)rs_total[2 * ((k / rs_d) * rescale.rows + k % rs_d) + 1]);
        if (wr && bam_writer_close(wr, err, sizeof err)) { fprintf(stderr, "hostcheck: %s\n", err); return 1; }
        const int32_t n_ref = rd ? bam_reader_header(rd)->n_ref : sam_reader_n_ref(sd);
        printf("alignments input=%s refs=%d records=%llu bytes=%llu digest=%016llx\n", is_bam ? "bam" : "sam", n_ref,
               (unsigned long long)recs, (unsigned long long)bytes, (unsigned long long)h);
        fprintf(stderr, "hostcheck: %llu batches\n", (unsigned long long)batches);
        if (rd) fprintf(stderr, "hostcheck: reader inflate stage %.3f s\n", bam_reader_inflate_seconds(rd));
        bam_reader_close(rd);
        sam_reader_close(sd);
    }
    if (genome) destroy_genome(genome);
    return 0;
}

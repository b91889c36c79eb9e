/*
 * pss-bam_amd/host/report.c -- the text the two tools emit.  These files are the
 * byte-for-byte parity surface; formats follow
 * /root/reference/pss-bam.c:504-633 and fragkon.c:231-249,:367-368.
 */
#include "report.h"
#include "composition.h"
#include "interior.h"
#include "pssbam_hip.h"

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#define PSS_VERSION "1.2.1"
#define FN_BUF 2047 /* the reference formats the output name into a MAX_FN_LEN buffer */

/* substitution rates per interior position: count / (column total of that reference base).
 * Column totals are summed as integers first, then divided in double, in the reference's
 * order, so "%.5e" prints identically.  A position whose A, C, G or T column is empty keeps
 * twelve zeros (pss-bam.c:512-514). */
void pss_sub_rates(int region_len, const unsigned long *counts, double *rates)
{
    /* cells of the twelve off-diagonal (read base, reference base) pairs; cell & 3 = reference base */
    static const unsigned char off_diag[12] = {1, 2, 3, 4, 6, 7, 8, 9, 11, 12, 13, 14};
    for (int pos = 0; pos < region_len; pos++) {
        const unsigned long *row = counts + (size_t)(pos + 2) * 16;
        double *out = rates + (size_t)pos * 12;
        double col[4];
        int empty = 0;
        for (int ref = 0; ref < 4; ref++) {
            unsigned long sum = row[ref] + row[4 + ref] + row[8 + ref] + row[12 + ref];
            col[ref] = sum;
            empty |= (sum == 0);
        }
        for (int j = 0; j < 12; j++) out[j] = empty ? 0.0 : row[off_diag[j]] / col[off_diag[j] & 3];
    }
}

static void count_row(FILE *fp, int label, const unsigned long *row)
{
    fprintf(fp, "%d\t", label);
    for (int j = 0; j < 16; j++) fprintf(fp, "%lu\t", row[j]); /* every row ends in a TAB */
    fputc('\n', fp);
}

int pss_write_counts(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len,
                     const unsigned long *fwd, const unsigned long *rev)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.counts.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    /* the counts header carries a literal "v1.2.1:" (with the colon) */
    fprintf(fp, "### pss-bam.c v1.2.1:\n### FASTA: %s\n### BAM: %s\n### OUT: %s\n", fasta_fn, bam_fn, fn);
    fputs("### Format of table:\n", fp);
    fputs("### Counts of how often a read base and genome base were seen at\n", fp);
    fputs("### each position in the aligned reads.\n", fp);
    fputs("### First base is what was seen in the read.\n", fp);
    fputs("### Second base is what was in the genome at that position.\n", fp);
    fputs("### POS AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT\n", fp);
    fputs("### Forward read substitution counts and base context\n", fp);
    for (int r = 0; r < region_len + 2; r++) count_row(fp, r - 2, fwd + (size_t)r * 16);
    /* two blank lines separate the gnuplot data sets */
    fputs("\n\n### Reverse read substitution counts and base context\n", fp);
    for (int pos = region_len - 1; pos >= 0; pos--) count_row(fp, pos, rev + (size_t)(pos + 2) * 16);
    count_row(fp, 1, rev + 16); /* first base past the alignment  */
    count_row(fp, 2, rev);      /* second base past the alignment */
    fclose(fp);
    return 0;
}

static void rate_row(FILE *fp, int label, const double *row)
{
    fprintf(fp, "%d\t", label);
    for (int j = 0; j < 12; j++) fprintf(fp, "%.5e\t", row[j]);
    fputc('\n', fp);
}

int pss_write_rates(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len,
                    const double *fwd_rates, const double *rev_rates)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.rates.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "### pss-bam.c v%s\n### FASTA: %s\n### BAM: %s\n### OUT: %s\n", PSS_VERSION, fasta_fn, bam_fn, fn);
    fputs("### Format of table:\n", fp);
    fputs("### Substitution rates for all possible nucleotide substitutions at\n", fp);
    fputs("### each position in the aligned reads.\n", fp);
    fputs("### First base is what was seen in the read.\n", fp);
    fputs("### Second base is what was in the genome at that position.\n", fp);
    fputs("### POS AC AG AT CA CG CT GA GC GT TA TC TG\n", fp);
    fputs("### Forward read substitution rates\n", fp);
    for (int pos = 0; pos < region_len; pos++) rate_row(fp, pos, fwd_rates + (size_t)pos * 12);
    fputs("\n\n### Reverse read substitution rates\n", fp);
    for (int pos = region_len - 1; pos >= 0; pos--) rate_row(fp, pos, rev_rates + (size_t)pos * 12);
    fclose(fp);
    return 0;
}

int pss_write_rates_se(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len, int k,
                       const double *fwd_se, const double *rev_se)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.rates.se.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "### pss-bam.c v%s\n### FASTA: %s\n### BAM: %s\n### OUT: %s\n", PSS_VERSION, fasta_fn, bam_fn, fn);
    fputs("### Format of table:\n", fp);
    fputs("### Substitution rates for all possible nucleotide substitutions at\n", fp);
    fputs("### each position in the aligned reads.\n", fp);
    fputs("### First base is what was seen in the read.\n", fp);
    fputs("### Second base is what was in the genome at that position.\n", fp);
    fputs("### POS AC AG AT CA CG CT GA GC GT TA TC TG\n", fp);
    fprintf(fp, "### jackknife standard errors of the forward read substitution rates, K = %d read-name replicates\n", k);
    for (int pos = 0; pos < region_len; pos++) rate_row(fp, pos, fwd_se + (size_t)pos * 12);
    fprintf(fp, "\n\n### jackknife standard errors of the reverse read substitution rates, K = %d read-name replicates\n", k);
    for (int pos = region_len - 1; pos >= 0; pos--) rate_row(fp, pos, rev_se + (size_t)pos * 12);
    return fclose(fp) ? 1 : 0;
}

int pss_write_labelled(const char *fasta_fn, const char *bam_fn, const char *out_prefix, const char *tag, int region_len,
                       const unsigned long *fwd, const unsigned long *rev)
{
    const size_t n_rates = (size_t)(region_len ? region_len : 1) * 12;
    char *prefix = (char *)malloc(strlen(out_prefix) + strlen(tag) + 2);
    double *fwd_rates = (double *)calloc(n_rates, sizeof(double)), *rev_rates = (double *)calloc(n_rates, sizeof(double));
    int rc = 1;
    if (prefix && fwd_rates && rev_rates) {
        sprintf(prefix, "%s.%s", out_prefix, tag);
        pss_sub_rates(region_len, fwd, fwd_rates);
        pss_sub_rates(region_len, rev, rev_rates);
        rc = pss_write_counts(fasta_fn, bam_fn, prefix, region_len, fwd, rev);
        rc |= pss_write_rates(fasta_fn, bam_fn, prefix, region_len, fwd_rates, rev_rates);
    } else fprintf(stderr, "Error: out of memory\n");
    free(prefix);
    free(fwd_rates);
    free(rev_rates);
    return rc;
}

static void contig_row(FILE *fp, const char *name, const char *table, int label, const unsigned long *row)
{
    fprintf(fp, "%s\t%s\t", name, table);
    count_row(fp, label, row);
}

int pss_write_contigs(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len, int n,
                      const char *const *names, const unsigned long *fwd, const unsigned long *rev)
{
    const size_t cells = (size_t)(region_len + 2) * 16;
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.contigs.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "### pss-bam.c v1.2.1:\n### FASTA: %s\n### BAM: %s\n### OUT: %s\n", fasta_fn, bam_fn, fn);
    fputs("### CONTIG TABLE POS AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT\n", fp);
    for (int k = 0; k < n; k++) {
        const unsigned long *f = fwd + (size_t)k * cells, *r = rev + (size_t)k * cells;
        for (int row = 0; row < region_len + 2; row++) contig_row(fp, names[k], "fwd", row - 2, f + (size_t)row * 16);
        for (int pos = region_len - 1; pos >= 0; pos--) contig_row(fp, names[k], "rev", pos, r + (size_t)(pos + 2) * 16);
        contig_row(fp, names[k], "rev", 1, r + 16);
        contig_row(fp, names[k], "rev", 2, r);
    }
    return fclose(fp) ? 1 : 0;
}

int pss_parse_end_condition(const char *arg, int *depth, int *cell5, int *cell3, char *err, size_t err_len)
{
    const int ss = strncmp(arg, "ss", 2) == 0, ds = strncmp(arg, "ds", 2) == 0;
    const char *rest = arg + 2;
    long d = 1;
    if (!ss && !ds) {
        snprintf(err, err_len, "-E (tables conditional on the other end): unknown preset in \"%s\"; give ss or ds, optionally \",<depth>\".", arg);
        return -1;
    }
    if (*rest) {
        char *end = NULL;
        if (*rest != ',' || rest[1] < '0' || rest[1] > '9' || (d = strtol(rest + 1, &end, 10), *end) || d < 1 || d > PSSBAM_MAX_END_DEPTH) {
            snprintf(err, err_len, "-E (tables conditional on the other end): bad depth in \"%s\"; give <ss|ds>[,<d>] with d in 1..%d.", arg,
                     PSSBAM_MAX_END_DEPTH);
            return -1;
        }
    }
    *depth = (int)d;
    *cell5 = 13;
    *cell3 = ss ? 13 : 2;
    return 0;
}

int pss_write_end_reads(const char *out_prefix, const uint64_t reads[4])
{
    static const char *const names[4] = {"unpaired_reads", "marked_5p", "marked_3p", "marked_both"};
    char *fn = (char *)malloc(strlen(out_prefix) + 32);
    if (!fn) { fprintf(stderr, "Error: out of memory\n"); return 1; }
    sprintf(fn, "%s.cond.pss.reads.txt", out_prefix);
    FILE *f = fopen(fn, "w");
    if (!f) {
        fprintf(stderr, "Error: unable to write %s\n", fn);
        free(fn);
        return 1;
    }
    for (int k = 0; k < 4; k++) fprintf(f, "%s\t%llu\n", names[k], (unsigned long long)reads[k]);
    free(fn);
    return fclose(f) ? 1 : 0;
}

int pss_write_lengths(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int max_len, const uint64_t *fwd,
                      const uint64_t *rev)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.lengths.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "# fragment lengths of the reads added to the forward / reverse table\n# FASTA: %s\n# BAM: %s\n", fasta_fn, bam_fn);
    fputs("length\tfwd\trev\n", fp);
    for (int len = 0; len <= max_len; len++)
        fprintf(fp, "%d\t%llu\t%llu\n", len, (unsigned long long)fwd[len], (unsigned long long)rev[len]);
    fprintf(fp, ">%d\t%llu\t%llu\n", max_len, (unsigned long long)fwd[max_len + 1], (unsigned long long)rev[max_len + 1]);
    return fclose(fp) ? 1 : 0;
}

int pss_write_mismatches(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int max_mm, int transversions_only,
                         const uint64_t *fwd, const uint64_t *rev)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.mismatches.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "# mismatches (%s) of the reads added to the forward / reverse table\n# FASTA: %s\n# BAM: %s\n",
            transversions_only ? "transversions only" : "all", fasta_fn, bam_fn);
    fputs("mismatches\tfwd\trev\n", fp);
    for (int m = 0; m <= max_mm; m++)
        fprintf(fp, "%d\t%llu\t%llu\n", m, (unsigned long long)fwd[m], (unsigned long long)rev[m]);
    fprintf(fp, ">%d\t%llu\t%llu\n", max_mm, (unsigned long long)fwd[max_mm + 1], (unsigned long long)rev[max_mm + 1]);
    return fclose(fp) ? 1 : 0;
}

int pss_write_interior(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int margin, int min_bq, const uint64_t table[16],
                       uint64_t reads)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.interior.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "# substitution counts and rates of the read interior: the positions at least %d bases from both ends of the tallied reads", margin);
    if (min_bq > 0) fprintf(fp, ", base quality at least %d (-Q %d)", min_bq, min_bq);
    fprintf(fp, "\n# FASTA: %s\n# BAM: %s\n", fasta_fn, bam_fn);
    unsigned long row[16];
    double rates[12];
    uint64_t bases = 0;
    for (int j = 0; j < 16; j++) {
        row[j] = (unsigned long)table[j];
        bases += table[j];
    }
    pss_interior_rates(table, rates);
    fputs("### POS AA AC AG AT CA CC CG CT GA GC GG GT TA TC TG TT\n", fp);
    count_row(fp, margin, row);
    fputs("### POS AC AG AT CA CG CT GA GC GT TA TC TG\n", fp);
    rate_row(fp, margin, rates);
    fprintf(fp, "reads\t%llu\nbases\t%llu\n", (unsigned long long)reads, (unsigned long long)bases);
    return fclose(fp) ? 1 : 0;
}

static void composition_row(FILE *fp, int label, const uint64_t *row)
{
    double frac[4];
    pss_composition_fractions(row, frac);
    fprintf(fp, "%d\t", label);
    for (int j = 0; j < 5; j++) fprintf(fp, "%lu\t", (unsigned long)row[j]); /* every row ends in a TAB */
    for (int j = 0; j < 4; j++) fprintf(fp, "%.5e\t", frac[j]);
    fputc('\n', fp);
}

int pss_write_composition(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int width, const uint64_t *c5,
                          const uint64_t *c3)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.composition.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "# reference base composition %d bases on either side of the ends of the tallied reads, in the read's orientation"
                " (negative: outside the read)\n", width);
    fprintf(fp, "# FASTA: %s\n# BAM: %s\n", fasta_fn, bam_fn);
    fputs("### POS A C G T other fA fC fG fT\n", fp);
    fputs("### Forward read base composition around the 5' end\n", fp);
    for (int j = -width; j < width; j++) composition_row(fp, j, c5 + (size_t)(j + width) * 5);
    /* two blank lines separate the gnuplot data sets; the 3' block mirrors the counts file: inside rows down to the end, then
     * the bases past the alignment labelled 1 .. width */
    fputs("\n\n### Reverse read base composition around the 3' end\n", fp);
    for (int j = width - 1; j >= 0; j--) composition_row(fp, j, c3 + (size_t)(j + width) * 5);
    for (int j = 1; j <= width; j++) composition_row(fp, j, c3 + (size_t)(width - j) * 5);
    return fclose(fp) ? 1 : 0;
}

int pss_write_read_scores(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int hist_half, const uint64_t *fwd,
                          const uint64_t *rev)
{
    char fn[FN_BUF + 1];
    FILE *fp;
    snprintf(fn, sizeof fn, "%s.pss.pmd.txt", out_prefix);
    fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        return 1;
    }
    fprintf(fp, "# post-mortem-damage score (whole nats, rounded down) of the reads added to the forward / reverse table\n# FASTA: %s\n# BAM: %s\n",
            fasta_fn, bam_fn);
    fputs("score\tfwd\trev\n", fp);
    fprintf(fp, "<%d\t%llu\t%llu\n", 1 - hist_half, (unsigned long long)fwd[0], (unsigned long long)rev[0]);
    for (int b = 1; b < 2 * hist_half - 1; b++)
        fprintf(fp, "%d\t%llu\t%llu\n", b - hist_half, (unsigned long long)fwd[b], (unsigned long long)rev[b]);
    fprintf(fp, ">=%d\t%llu\t%llu\n", hist_half - 1, (unsigned long long)fwd[2 * hist_half - 1], (unsigned long long)rev[2 * hist_half - 1]);
    return fclose(fp) ? 1 : 0;
}

int fragkon_write_table(FILE *out, const char *fasta_fn, const char *bam_fn, int klen, const uint64_t *k5,
                        const uint64_t *k3)
{
    const uint64_t bins = (uint64_t)1 << (2 * klen);
    char kmer[40];
    if (klen < 1 || klen > 31) return 1;
    fprintf(out, "### fragkon.c v0.3\n### %s\n### %s\n", fasta_fn, bam_fn);
    fprintf(out, "# KMER\t5' CONTEXT COUNTS\t3' CONTEXT COUNTS\n");
    kmer[klen] = '\0';
    /* ACGT-lexicographic enumeration == ascending bin index */
    for (uint64_t b = 0; b < bins; b++) {
        for (int i = 0; i < klen; i++) kmer[i] = "ACGT"[(b >> (2 * (klen - 1 - i))) & 3u];
        unsigned int c5 = k5[b] > UINT_MAX ? UINT_MAX : (unsigned int)k5[b]; /* counts stick at UINT_MAX */
        unsigned int c3 = k3[b] > UINT_MAX ? UINT_MAX : (unsigned int)k3[b];
        fprintf(out, "%s\t%u\t%u\n", kmer, c5, c3);
    }
    return 0;
}

int fragkon_write_plane(const char *fasta_fn, const char *bam_fn, const char *out_prefix, const char *tag, int klen,
                        const uint64_t *k5, const uint64_t *k3)
{
    const size_t cap = strlen(out_prefix) + strlen(tag) + sizeof "..fragkon.txt";
    char *fn = (char *)malloc(cap);
    if (!fn) {
        fprintf(stderr, "Error: out of memory\n");
        return 1;
    }
    snprintf(fn, cap, "%s.%s.fragkon.txt", out_prefix, tag);
    FILE *fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        free(fn);
        return 1;
    }
    int rc = fragkon_write_table(fp, fasta_fn, bam_fn, klen, k5, k3);
    if (fclose(fp)) rc = 1;
    free(fn);
    return rc;
}

/* genome-kmer-count's table (/root/reference/genome-kmer-count.c:56-66 prints kmer2count(): an
 * unsigned int that sticks at UINT_MAX, kmer.c:102-104) */
int gkc_write_table(FILE *out, int klen, const uint64_t *counts)
{
    const uint64_t bins = (uint64_t)1 << (2 * klen);
    char kmer[40];
    if (klen < 1 || klen > 31) return 1;
    kmer[klen] = '\0';
    for (uint64_t b = 0; b < bins; b++) {
        for (int i = 0; i < klen; i++) kmer[i] = "ACGT"[(b >> (2 * (klen - 1 - i))) & 3u];
        fprintf(out, "%s\t%u\n", kmer, counts[b] > UINT_MAX ? UINT_MAX : (unsigned int)counts[b]);
    }
    return 0;
}

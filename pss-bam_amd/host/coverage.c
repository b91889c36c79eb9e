/* pss-bam_amd/host/coverage.c -- see coverage.h */
#include "coverage.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static double ratio(uint64_t a, uint64_t b) { return b ? (double)a / (double)b : 0.0; }

int pss_write_coverage(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int n, const char *const *names, const uint8_t *held,
                       const uint64_t *lengths, const uint64_t *per_contig, const uint64_t *hist, int hist_max)
{
    char *fn = (char *)malloc(strlen(out_prefix) + 32);
    if (!fn) { fprintf(stderr, "Error: out of memory\n"); return 1; }
    sprintf(fn, "%s.pss.coverage.txt", out_prefix);
    FILE *fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        free(fn);
        return 1;
    }
    free(fn);
    fprintf(fp, "# depth of coverage of the tallied reads: every read added to a table covers POS .. POS + length - 1 of its contig\n"
                "# FASTA: %s\n# BAM: %s\n", fasta_fn, bam_fn);
    fputs("contig\tlength\tcovered_bases\tbreadth\tdepth_sum\tmean_depth\tmax_depth\n", fp);
    uint64_t t_len = 0, t_cov = 0, t_sum = 0, t_max = 0;
    for (int i = 0; i < n; i++) {
        if (!held[i]) continue;
        const uint64_t *p = per_contig + 3 * (size_t)i;
        fprintf(fp, "%s\t%llu\t%llu\t%.6f\t%llu\t%.6f\t%llu\n", names[i], (unsigned long long)lengths[i], (unsigned long long)p[0], ratio(p[0], lengths[i]),
                (unsigned long long)p[1], ratio(p[1], lengths[i]), (unsigned long long)p[2]);
        t_len += lengths[i];
        t_cov += p[0];
        t_sum += p[1];
        if (p[2] > t_max) t_max = p[2];
    }
    fprintf(fp, "total\t%llu\t%llu\t%.6f\t%llu\t%.6f\t%llu\n", (unsigned long long)t_len, (unsigned long long)t_cov, ratio(t_cov, t_len),
            (unsigned long long)t_sum, ratio(t_sum, t_len), (unsigned long long)t_max);
    fputs("depth\tpositions\n", fp);
    for (int d = 0; d <= hist_max; d++) fprintf(fp, "%d\t%llu\n", d, (unsigned long long)hist[d]);
    fprintf(fp, ">%d\t%llu\n", hist_max, (unsigned long long)hist[hist_max + 1]);
    return fclose(fp) ? 1 : 0;
}

int pss_write_coverage_bedgraph(const char *path, int n, const char *const *names, uint64_t n_runs, const int32_t *ref, const uint32_t *start,
                                const uint32_t *end, const uint32_t *depth)
{
    char *tmp = (char *)malloc(strlen(path) + 8);
    if (!tmp) { fprintf(stderr, "Error: out of memory\n"); return 1; }
    sprintf(tmp, "%s.tmp", path);
    FILE *fp = fopen(tmp, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", tmp);
        free(tmp);
        return 1;
    }
    int bad = 0;
    for (uint64_t i = 0; i < n_runs && !bad; i++) {
        if (ref[i] < 0 || ref[i] >= n) { fprintf(stderr, "Error: coverage run %llu names reference %d of %d\n", (unsigned long long)i, (int)ref[i], n); bad = 1; break; }
        if (fprintf(fp, "%s\t%u\t%u\t%u\n", names[ref[i]], start[i], end[i], depth[i]) < 0) bad = 1;
    }
    if (fclose(fp)) bad = 1;
    if (!bad && rename(tmp, path)) bad = 1;
    if (bad) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", path);
        remove(tmp);
    }
    free(tmp);
    return bad;
}

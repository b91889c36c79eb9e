/* pss-bam_amd/host/windows.c -- see windows.h */
#include "windows.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static double ratio(uint64_t a, uint64_t b) { return b ? (double)a / (double)b : 0.0; }

int pss_parse_window(const char *arg, uint32_t *window)
{
    if (!arg || *arg < '0' || *arg > '9') return 1;
    uint64_t v = 0;
    for (const char *p = arg; *p; p++) {
        if (*p < '0' || *p > '9') return 1;
        v = v * 10 + (uint64_t)(*p - '0');
        if (v > PSS_WINDOW_MAX) return 1;
    }
    if (v < PSS_WINDOW_MIN) return 1;
    *window = (uint32_t)v;
    return 0;
}

uint64_t pss_gcbias_rows(uint32_t window, uint64_t n, const uint32_t *start, const uint32_t *end, const uint32_t *acgt, const uint32_t *gc,
                         const uint64_t *depth_sum, uint64_t *bin_windows, uint64_t *bin_depth_sum)
{
    uint64_t used = 0;
    for (int b = 0; b < PSS_GC_BINS; b++) bin_windows[b] = bin_depth_sum[b] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (end[i] - start[i] != window || 2 * (uint64_t)acgt[i] < window || !acgt[i]) continue;
        if (gc[i] > acgt[i]) continue;   /* (never from the engine: gc counts some of acgt's letters; a bin beyond 100 has no row) */
        const uint64_t b = (200 * (uint64_t)gc[i] + acgt[i]) / (2 * (uint64_t)acgt[i]);
        bin_windows[b]++;
        bin_depth_sum[b] += depth_sum[i];
        used++;
    }
    return used;
}

static FILE *open_tmp(const char *out_prefix, const char *suffix, char **tmp, char **path)
{
    const size_t room = strlen(out_prefix) + strlen(suffix) + 8;
    *tmp = (char *)malloc(room);
    *path = (char *)malloc(room);
    if (!*tmp || !*path) { fprintf(stderr, "Error: out of memory\n"); return NULL; }
    sprintf(*path, "%s%s", out_prefix, suffix);
    sprintf(*tmp, "%s.tmp", *path);
    return fopen(*tmp, "w");   /* (the caller says what failed) */
}

int pss_write_windows(const char *fasta_fn, const char *bam_fn, const char *out_prefix, uint32_t window, int n_names, const char *const *names,
                      uint64_t n, const int32_t *ref, const uint32_t *start, const uint32_t *end, const uint32_t *acgt, const uint32_t *gc,
                      const uint32_t *covered, const uint64_t *depth_sum)
{
    char *w_tmp = NULL, *w_path = NULL, *g_tmp = NULL, *g_path = NULL;
    int bad = 0, w_made = 0, g_made = 0, said = 0;
    const char *failed = NULL;   /* the file that could not be written */
    FILE *fp = open_tmp(out_prefix, ".pss.windows.txt", &w_tmp, &w_path);
    if (!fp) { bad = 1; failed = w_tmp; }
    if (!bad) {
        w_made = 1;
        fprintf(fp, "# fixed windows over the depth of coverage of the tallied reads: the FASTA's A/C/G/T and C/G letters, the covered positions and the summed depth of each\n"
                    "# FASTA: %s\n# BAM: %s\n# window: %u\n# windows: %llu\n", fasta_fn, bam_fn, window, (unsigned long long)n);
        fputs("contig\tstart\tend\tacgt\tgc\tgc_fraction\tcovered\tdepth_sum\tmean_depth\n", fp);
        for (uint64_t i = 0; i < n && !bad; i++) {
            if (ref[i] < 0 || ref[i] >= n_names) { fprintf(stderr, "Error: window %llu names reference %d of %d\n", (unsigned long long)i, (int)ref[i], n_names); bad = said = 1; break; }
            char frac[32];
            if (acgt[i]) snprintf(frac, sizeof frac, "%.6f", (double)gc[i] / (double)acgt[i]);
            else strcpy(frac, "NA");
            if (fprintf(fp, "%s\t%u\t%u\t%u\t%u\t%s\t%u\t%llu\t%.6f\n", names[ref[i]], start[i], end[i], acgt[i], gc[i], frac, covered[i],
                        (unsigned long long)depth_sum[i], ratio(depth_sum[i], (uint64_t)(end[i] - start[i]))) < 0) bad = 1;
        }
        if (fclose(fp)) bad = 1;
        if (bad) failed = w_tmp;
    }
    if (!bad) {
        fp = open_tmp(out_prefix, ".pss.gcbias.txt", &g_tmp, &g_path);
        if (!fp) { bad = 1; failed = g_tmp; }
    }
    if (!bad) {
        g_made = 1;
        uint64_t bw[PSS_GC_BINS], bs[PSS_GC_BINS], t_sum = 0;
        const uint64_t used = pss_gcbias_rows(window, n, start, end, acgt, gc, depth_sum, bw, bs);
        for (int b = 0; b < PSS_GC_BINS; b++) t_sum += bs[b];
        const double overall = ratio(t_sum, used * window);
        fprintf(fp, "# GC bias of the tallied reads: the windows of the full size with at least half of their letters A, C, G or T, by the GC percentage of those letters (rounded half up)\n"
                    "# FASTA: %s\n# BAM: %s\n# window: %u\n# windows: %llu\n# used windows: %llu\n# mean depth of the used windows: %.6f\n", fasta_fn, bam_fn, window,
                (unsigned long long)n, (unsigned long long)used, overall);
        fputs("gc_percent\twindows\tpositions\tdepth_sum\tmean_depth\trelative_depth\n", fp);
        for (int b = 0; b < PSS_GC_BINS; b++) {
            const double mean = ratio(bs[b], bw[b] * window);
            if (fprintf(fp, "%d\t%llu\t%llu\t%llu\t%.6f\t%.6f\n", b, (unsigned long long)bw[b], (unsigned long long)(bw[b] * window), (unsigned long long)bs[b], mean,
                        overall > 0.0 ? mean / overall : 0.0) < 0) bad = 1;
        }
        if (fclose(fp)) bad = 1;
        if (bad) failed = g_tmp;
    }
    if (!bad && rename(w_tmp, w_path)) { bad = 1; failed = w_path; }
    if (!bad) {
        w_made = 0;
        if (rename(g_tmp, g_path)) { bad = 1; failed = g_path; remove(w_path); }
        else g_made = 0;
    }
    if (bad) {
        if (!said) fprintf(stderr, "ERROR: Cannot write to file %s\n.", failed ? failed : out_prefix);
        if (w_made) remove(w_tmp);
        if (g_made) remove(g_tmp);
    }
    free(w_tmp); free(w_path); free(g_tmp); free(g_path);
    return bad;
}

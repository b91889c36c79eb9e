/* pss-bam_amd/host/duplicates.c -- see duplicates.h */
#include "duplicates.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int pss_write_duplicates(const char *fasta_fn, const char *bam_fn, const char *out_prefix, const char *tool, const uint64_t totals[3],
                         const uint64_t *hist, int hist_max)
{
    char *fn = (char *)malloc(strlen(out_prefix) + strlen(tool) + 32);
    if (!fn) { fprintf(stderr, "Error: out of memory\n"); return 1; }
    sprintf(fn, "%s.%s.duplicates.txt", out_prefix, tool);
    FILE *fp = fopen(fn, "w");
    if (!fp) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        free(fn);
        return 1;
    }
    free(fn);
    fprintf(fp, "# duplicates among the unpaired candidate reads: same contig, position, length, strand and read group; the first in input order is kept\n"
                "# FASTA: %s\n# BAM: %s\n", fasta_fn, bam_fn);
    fprintf(fp, "eligible_reads\t%llu\n", (unsigned long long)totals[0]);
    fprintf(fp, "distinct_keys\t%llu\n", (unsigned long long)totals[1]);
    fprintf(fp, "flagged_reads\t%llu\n", (unsigned long long)totals[2]);
    fprintf(fp, "duplicate_fraction\t%.6f\n", totals[0] ? (double)totals[2] / (double)totals[0] : 0.0);
    fputs("size\tgroups\n", fp);
    for (int c = 1; c <= hist_max; c++) fprintf(fp, "%d\t%llu\n", c, (unsigned long long)hist[c]);
    fprintf(fp, ">%d\t%llu\n", hist_max, (unsigned long long)hist[hist_max + 1]);
    return fclose(fp) ? 1 : 0;
}

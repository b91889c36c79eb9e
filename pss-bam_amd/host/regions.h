/* pss-bam_amd/host/regions.h -- pss-bam -T / fragkon -T: the BED reader (exported from libpssbam_host.so). */
#ifndef PSSBAM_REGIONS_H
#define PSSBAM_REGIONS_H
#include <stddef.h>
#include <stdint.h>

/* The intervals of a BED file in the form pssbam_engine_set_regions takes: interval i is [starts[i], ends[i]) on
 * names[name_of[i]] (every name once, in order of first appearance). */
typedef struct pss_regions {
    int32_t n_names;
    char **names;
    int64_t n;
    int32_t *name_of;
    uint32_t *starts, *ends;
} pss_regions;

/* Parses plain-text BED: fields separated by blanks or tabs, the first three used (contig, 0-based start, end;
 * half open).  Empty lines and lines that start with '#', "track" or "browser" are skipped.  Returns 0 and fills
 * *out (pss_free_regions), or -1 with a one-line diagnostic (no newline, with the line number where there is one) in
 * err[0..err_cap): fewer than three fields, a coordinate that is not a decimal integer or is 2^32 or above,
 * start > end, more than PSSBAM_MAX_REGIONS intervals, or no interval at all. */
int pss_parse_bed(const char *text, size_t len, pss_regions *out, char *err, size_t err_cap);
/* The same for a file; an unreadable file is an error too. */
int pss_read_bed(const char *path, pss_regions *out, char *err, size_t err_cap);
void pss_free_regions(pss_regions *r);
#endif

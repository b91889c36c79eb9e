/* pss-bam_amd/host/length_bins.h -- pss-bam -S helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_LENGTH_BINS_H
#define PSSBAM_LENGTH_BINS_H
#include <stddef.h>
#include <stdint.h>

/* The -S argument "e1,e2,...,ek": decimal integers (digits only: no sign, no blanks, no empty item) with
 * min_len < e1 < e2 < ... < ek <= min(max_len, 2^32-1) and 1 <= k <= 63 (PSSBAM_MAX_LENGTH_BINS - 1).  min_len
 * and max_len are the -l / -L values in effect.  Writes the edges to edges[0..k-1] (room for 63) and returns k,
 * or -1 with a one-line diagnostic (no newline) in err[0..err_cap). */
int pss_parse_length_edges(const char *arg, unsigned long min_len, unsigned long max_len, uint32_t *edges, char *err,
                           size_t err_cap);
/* The file-name tag of the bin [lo, hi]: "len<lo>-<hi>".  Writes at most cap-1 bytes + NUL; returns the full
 * length (without the NUL). */
size_t pss_length_bin_tag(unsigned long lo, unsigned long hi, char *out, size_t cap);
/* Bounds of bin b of k edges: [min_len, e1-1], [e1, e2-1], ..., [ek, max_len]. */
void pss_length_bin_bounds(const uint32_t *edges, int k, int b, unsigned long min_len, unsigned long max_len,
                           unsigned long *lo, unsigned long *hi);
#endif

/*
 * pss-bam_amd/host/length_bins.c -- pss-bam -S: the edge list of the length bins and the file-name tag
 * of a bin.
 */
#include "length_bins.h"

#include <stdio.h>

#define MAX_EDGES 63

int pss_parse_length_edges(const char *arg, unsigned long min_len, unsigned long max_len, uint32_t *edges, char *err,
                           size_t err_cap)
{
    const unsigned long long top = max_len < 4294967295ul ? max_len : 4294967295ul;
    int k = 0;
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-S needs a comma-separated list of length bin edges");
        return -1;
    }
    for (const char *p = arg;;) {
        const char *q = p;
        unsigned long long v = 0;
        while (*q >= '0' && *q <= '9') {
            v = v * 10 + (unsigned long long)(*q - '0');
            if (v > 4294967295ull) break;
            q++;
        }
        if (q == p || (*q != ',' && *q != '\0')) {
            if (q != p && *q >= '0' && *q <= '9')
                snprintf(err, err_cap, "-S: edge %d is larger than 4294967295", k + 1);
            else
                snprintf(err, err_cap, "-S: edge %d is not a decimal integer (edges are digits separated by commas)", k + 1);
            return -1;
        }
        if (k == MAX_EDGES) {
            snprintf(err, err_cap, "-S: more than %d edges (at most %d length bins)", MAX_EDGES, MAX_EDGES + 1);
            return -1;
        }
        if (k > 0 && v <= edges[k - 1]) {
            snprintf(err, err_cap, "-S: edge %d (%llu) does not rise above edge %d (%u)", k + 1, v, k, edges[k - 1]);
            return -1;
        }
        if (v <= min_len || v > top) {
            snprintf(err, err_cap, "-S: edge %d (%llu) lies outside (%lu, %llu], the -l / -L range", k + 1, v, min_len, top);
            return -1;
        }
        edges[k++] = (uint32_t)v;
        if (*q == '\0') return k;
        p = q + 1;
    }
}

size_t pss_length_bin_tag(unsigned long lo, unsigned long hi, char *out, size_t cap)
{
    char tmp[64];
    const int n = snprintf(tmp, sizeof tmp, "len%lu-%lu", lo, hi);
    if (cap) snprintf(out, cap, "%s", tmp);
    return (size_t)n;
}

void pss_length_bin_bounds(const uint32_t *edges, int k, int b, unsigned long min_len, unsigned long max_len,
                           unsigned long *lo, unsigned long *hi)
{
    *lo = b == 0 ? min_len : edges[b - 1];
    *hi = b == k ? max_len : (unsigned long)edges[b] - 1;
}

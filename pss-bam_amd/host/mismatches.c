/*
 * pss-bam_amd/host/mismatches.c -- pss-bam -n / -N: the mismatch limit of the filter and of the histogram.
 */
#include "mismatches.h"

#include <stdio.h>

#define MAX_MISMATCHES 255

/* digits only, lo..MAX_MISMATCHES; `what` names the value in the diagnostics */
static int parse_count(const char *arg, char opt, const char *what, int lo, char *err, size_t err_cap)
{
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-%c needs %s (%d..%d)", opt, what, lo, MAX_MISMATCHES);
        return -1;
    }
    int v = 0;
    const char *q = arg;
    while (*q >= '0' && *q <= '9') {
        v = v * 10 + (*q - '0');
        if (v > MAX_MISMATCHES) break;
        q++;
    }
    if (*q >= '0' && *q <= '9') {
        snprintf(err, err_cap, "-%c: %s is above %d (%d..%d)", opt, what, MAX_MISMATCHES, lo, MAX_MISMATCHES);
        return -1;
    }
    if (*q != '\0') {
        snprintf(err, err_cap, "-%c: %s is not a decimal integer (digits only, %d..%d)", opt, what, lo, MAX_MISMATCHES);
        return -1;
    }
    if (v < lo) {
        snprintf(err, err_cap, "-%c: %s must be at least %d (%d..%d)", opt, what, lo, lo, MAX_MISMATCHES);
        return -1;
    }
    return v;
}

int pss_parse_max_mismatches(const char *arg, char *err, size_t err_cap)
{
    return parse_count(arg, 'n', "the largest mismatch count of a tallied read", 0, err, err_cap);
}

int pss_parse_mismatch_hist(const char *arg, char *err, size_t err_cap)
{
    return parse_count(arg, 'N', "the largest mismatch count to list", 1, err, err_cap);
}

/*
 * pss-bam_amd/host/base_quality.c -- pss-bam -Q: the minimum base quality argument.
 */
#include "base_quality.h"

#include <stdio.h>

#define MAX_Q 93

int pss_parse_min_base_quality(const char *arg, char *err, size_t err_cap)
{
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-Q needs a minimum base quality (a Phred value, 0..%d)", MAX_Q);
        return -1;
    }
    int v = 0;
    const char *q = arg;
    while (*q >= '0' && *q <= '9') {
        v = v * 10 + (*q - '0');
        if (v > MAX_Q) break;
        q++;
    }
    if (*q >= '0' && *q <= '9') {
        snprintf(err, err_cap, "-Q: the minimum base quality is larger than %d, the largest Phred value a SAM file can hold", MAX_Q);
        return -1;
    }
    if (*q != '\0') {
        snprintf(err, err_cap, "-Q: the minimum base quality is not a decimal integer (digits only, 0..%d)", MAX_Q);
        return -1;
    }
    return v;
}

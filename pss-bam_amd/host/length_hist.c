/*
 * pss-bam_amd/host/length_hist.c -- pss-bam -H: the limit of the fragment-length histogram.
 */
#include "length_hist.h"

#include <stdio.h>

#define MAX_LEN 65535

int pss_parse_length_hist(const char *arg, char *err, size_t err_cap)
{
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-H needs the largest fragment length to list (1..%d)", MAX_LEN);
        return -1;
    }
    int v = 0;
    const char *q = arg;
    while (*q >= '0' && *q <= '9') {
        v = v * 10 + (*q - '0');
        if (v > MAX_LEN) break;
        q++;
    }
    if (*q >= '0' && *q <= '9') {
        snprintf(err, err_cap, "-H: the largest fragment length is above %d; longer reads share the last row anyway", MAX_LEN);
        return -1;
    }
    if (*q != '\0') {
        snprintf(err, err_cap, "-H: the largest fragment length is not a decimal integer (digits only, 1..%d)", MAX_LEN);
        return -1;
    }
    if (v < 1) {
        snprintf(err, err_cap, "-H: the largest fragment length must be at least 1 (1..%d)", MAX_LEN);
        return -1;
    }
    return v;
}

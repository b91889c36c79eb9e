/*
 * pss-bam_amd/host/composition.c -- pss-bam -P: the width argument and the base fractions of a row of the composition table.
 */
#include "composition.h"

#include <stdio.h>

#define MAX_COMPOSITION 30

int pss_parse_composition_width(const char *arg, char *err, size_t err_cap)
{
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-P needs the number of bases on either side of a read end (1..%d)", MAX_COMPOSITION);
        return -1;
    }
    int v = 0;
    const char *q = arg;
    while (*q >= '0' && *q <= '9') {
        v = v * 10 + (*q - '0');
        if (v > MAX_COMPOSITION) break;
        q++;
    }
    if (*q >= '0' && *q <= '9') {
        snprintf(err, err_cap, "-P: the width is above %d (1..%d)", MAX_COMPOSITION, MAX_COMPOSITION);
        return -1;
    }
    if (*q != '\0') {
        snprintf(err, err_cap, "-P: the width is not a decimal integer (digits only, 1..%d)", MAX_COMPOSITION);
        return -1;
    }
    if (v < 1) {
        snprintf(err, err_cap, "-P: the width is below 1 (1..%d)", MAX_COMPOSITION);
        return -1;
    }
    return v;
}

void pss_composition_fractions(const uint64_t row[5], double frac[4])
{
    const uint64_t sum = row[0] + row[1] + row[2] + row[3];
    for (int b = 0; b < 4; b++) frac[b] = sum ? (double)row[b] / (double)sum : 0.0;
}

/*
 * pss-bam_amd/host/interior.c -- pss-bam -W: the margin argument and the rates of the interior table.
 */
#include "interior.h"

#include <stdio.h>

#include "report.h"

#define MAX_INTERIOR_MARGIN 65535

int pss_parse_interior_margin(const char *arg, char *err, size_t err_cap)
{
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-W needs the margin left out at both ends of a read (0..%d)", MAX_INTERIOR_MARGIN);
        return -1;
    }
    int v = 0;
    const char *q = arg;
    while (*q >= '0' && *q <= '9') {
        v = v * 10 + (*q - '0');
        if (v > MAX_INTERIOR_MARGIN) break;
        q++;
    }
    if (*q >= '0' && *q <= '9') {
        snprintf(err, err_cap, "-W: the margin is above %d (0..%d)", MAX_INTERIOR_MARGIN, MAX_INTERIOR_MARGIN);
        return -1;
    }
    if (*q != '\0') {
        snprintf(err, err_cap, "-W: the margin is not a decimal integer (digits only, 0..%d)", MAX_INTERIOR_MARGIN);
        return -1;
    }
    return v;
}

void pss_interior_rates(const uint64_t table[16], double rates[12])
{
    /* one position of a table with the two context rows in front of it: the rule is pss_sub_rates' own */
    unsigned long rows[3 * 16] = {0};
    for (int j = 0; j < 16; j++) rows[32 + j] = (unsigned long)table[j];
    pss_sub_rates(1, rows, rates);
}

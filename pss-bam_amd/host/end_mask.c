/*
 * pss-bam_amd/host/end_mask.c -- pss-bam -K: the mode and the widths of the end mask.
 */
#include "end_mask.h"

#include <stdio.h>
#include <string.h>

#define MAX_N 65535

/* digits up to `stop` (',' or NUL); -1: empty or not digits, -2: above MAX_N */
static long width(const char **p)
{
    const char *q = *p;
    long v = 0;
    if (*q < '0' || *q > '9') return -1;
    while (*q >= '0' && *q <= '9') {
        v = v * 10 + (*q - '0');
        if (v > MAX_N) return -2;
        q++;
    }
    if (*q != '\0' && *q != ',') return -1;
    *p = q;
    return v;
}

int pss_parse_end_mask(const char *arg, int *mode, uint32_t *n5, uint32_t *n3, char *err, size_t err_cap)
{
    static const char *const names[] = {"all", "ds", "ss"};
    const char *comma = arg ? strchr(arg, ',') : NULL;
    const size_t len = arg ? (comma ? (size_t)(comma - arg) : strlen(arg)) : 0;
    int m = 0;
    for (int k = 0; k < 3; k++)
        if (strlen(names[k]) == len && !strncmp(arg, names[k], len)) m = k + 1;
    if (!m) {
        snprintf(err, err_cap, "-K: unknown mode \"%.*s\"; the modes are all, ds and ss (-K <mode>,<n5>[,<n3>])", (int)(len > 40 ? 40 : len), arg ? arg : "");
        return -1;
    }
    if (!comma) {
        snprintf(err, err_cap, "-K %s needs the number of bases to mask at the ends (-K <mode>,<n5>[,<n3>], 0..%d)", names[m - 1], MAX_N);
        return -1;
    }
    long v[2] = {0, 0};
    const char *q = comma + 1;
    int n = 0;
    for (; n < 2; n++) {
        v[n] = width(&q);
        if (v[n] == -2) {
            snprintf(err, err_cap, "-K: a width is above %d", MAX_N);
            return -1;
        }
        if (v[n] < 0) {
            snprintf(err, err_cap, "-K: the widths are decimal integers (digits only, 0..%d): -K <mode>,<n5>[,<n3>]", MAX_N);
            return -1;
        }
        if (*q == '\0') { n++; break; }
        q++;   /* the comma */
    }
    if (*q != '\0' || (n == 2 && q[-1] == ',')) {
        snprintf(err, err_cap, "-K takes a mode and one or two widths: -K <mode>,<n5>[,<n3>]");
        return -1;
    }
    if (n == 1) v[1] = v[0];
    if (v[0] == 0 && v[1] == 0) {
        snprintf(err, err_cap, "-K: both widths are 0: nothing to mask");
        return -1;
    }
    *mode = m;
    *n5 = (uint32_t)v[0];
    *n3 = (uint32_t)v[1];
    return 0;
}

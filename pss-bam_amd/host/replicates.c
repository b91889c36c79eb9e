/*
 * pss-bam_amd/host/replicates.c -- pss-bam -J: the replicate count, the read-name hash that picks a record's
 * replicate (restated from csrc/record_decode.h) and the jackknife over the replicates' tables.
 */
#include "replicates.h"
#include "report.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#define MAX_REPLICATES 64

int pss_parse_replicates(const char *arg, char *err, size_t err_cap)
{
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-J needs the number of read-name replicates (2..%d)", MAX_REPLICATES);
        return -1;
    }
    int v = 0;
    const char *q = arg;
    while (*q >= '0' && *q <= '9') {
        v = v * 10 + (*q - '0');
        if (v > MAX_REPLICATES) break;
        q++;
    }
    if (*q >= '0' && *q <= '9') {
        snprintf(err, err_cap, "-J: the number of read-name replicates is above %d (2..%d)", MAX_REPLICATES, MAX_REPLICATES);
        return -1;
    }
    if (*q != '\0') {
        snprintf(err, err_cap, "-J: the number of read-name replicates is not a decimal integer (digits only, 2..%d)", MAX_REPLICATES);
        return -1;
    }
    if (v < 2) {
        snprintf(err, err_cap, "-J: the number of read-name replicates must be at least 2 (2..%d)", MAX_REPLICATES);
        return -1;
    }
    return v;
}

uint32_t pss_read_name_hash(const uint8_t *name, size_t n)
{
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; i += 4) {
        uint32_t w = 0;
        for (size_t b = 0; b < 4 && i + b < n; b++) w |= (uint32_t)name[i + b] << (8 * b);
        h = (h ^ w) * 16777619u;
    }
    h ^= (uint32_t)n;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

int pss_read_name_replicate(const uint8_t *name, size_t n, int k)
{
    return (int)(((uint64_t)pss_read_name_hash(name, n) * (uint64_t)k) >> 32);
}

int pss_jackknife_se(int region_len, int k, const unsigned long *total, const unsigned long *planes, double *se_out)
{
    const size_t cells = (size_t)(region_len + 2) * 16, n_rates = (size_t)region_len * 12;
    unsigned long *rest = (unsigned long *)malloc(cells * sizeof *rest);
    double *theta = (double *)calloc((n_rates ? n_rates : 1) * (size_t)k, sizeof *theta);
    if (!rest || !theta) {
        free(rest);
        free(theta);
        return 1;
    }
    for (int j = 0; j < k; j++) {
        for (size_t i = 0; i < cells; i++) rest[i] = total[i] - planes[(size_t)j * cells + i];
        pss_sub_rates(region_len, rest, theta + (size_t)j * n_rates);
    }
    for (size_t i = 0; i < n_rates; i++) {
        double mean = 0.0, ss = 0.0;
        for (int j = 0; j < k; j++) mean += theta[(size_t)j * n_rates + i];
        mean /= k;
        for (int j = 0; j < k; j++) {
            const double d = theta[(size_t)j * n_rates + i] - mean;
            ss += d * d;
        }
        se_out[i] = sqrt((double)(k - 1) / k * ss);
    }
    free(rest);
    free(theta);
    return 0;
}

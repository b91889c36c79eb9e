/* pss-bam_amd/host/replicates.h -- pss-bam -J helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_REPLICATES_H
#define PSSBAM_REPLICATES_H
#include <stddef.h>
#include <stdint.h>

/* The -J argument: the number of read-name replicates, 2..64 (PSSBAM_MAX_REPLICATES) as a decimal integer -- digits
 * only: no sign, no blanks, not empty.  Returns the value, or -1 with a one-line diagnostic (no newline) in
 * err[0..err_cap). */
int pss_parse_replicates(const char *arg, char *err, size_t err_cap);

/* The replicate among k of a read named name[0..n) -- the bytes as a BAM record stores them, without the closing NUL;
 * an embedded NUL is a byte like any other.  The C restatement of what the tally kernels compute (include/pssbam_hip.h,
 * pssbam_engine_set_replicates), used by nothing on the hot path:
 *     h = 2166136261;  per four bytes, little endian, the last word zero-filled: h = (h ^ w) * 16777619;
 *     h ^= n;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16;  replicate = (h * k) >> 32
 * pss_read_name_hash returns h itself. */
uint32_t pss_read_name_hash(const uint8_t *name, size_t n);
int pss_read_name_replicate(const uint8_t *name, size_t n, int k);

/* The delete-one-group jackknife standard error of every rate pss_sub_rates gives for `total`.  total = one table of
 * (region_len + 2) * 16 counts, planes = the k replicate tables of the same size back to back, which add up to total.
 * With theta_j = pss_sub_rates(total - planes[j]) -- the function as it is, a position with an empty reference column
 * gives twelve zeros -- and mean = sum_j theta_j / k:
 *     se_out[pos * 12 + c] = sqrt((k - 1) / k * sum_j (theta_j - mean)^2)
 * se_out holds region_len * 12 doubles.  Returns 0, or 1 when memory runs out. */
int pss_jackknife_se(int region_len, int k, const unsigned long *total, const unsigned long *planes, double *se_out);
#endif

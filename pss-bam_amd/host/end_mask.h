/* pss-bam_amd/host/end_mask.h -- pss-bam -K helper (exported from libpssbam_host.so). */
#ifndef PSSBAM_END_MASK_H
#define PSSBAM_END_MASK_H
#include <stddef.h>
#include <stdint.h>

/* The -K argument, <mode>,<n5>[,<n3>]: mode is all, ds or ss (PSSBAM_END_MASK_ALL / _DS / _SS), the widths are decimal integers
 * 0..65535 (PSSBAM_MAX_END_MASK) -- digits only: no sign, no blanks, not empty --, n3 defaults to n5, and one of them is not 0.
 * Returns 0, or -1 with a one-line diagnostic (no newline) in err[0..err_cap). */
int pss_parse_end_mask(const char *arg, int *mode, uint32_t *n5, uint32_t *n3, char *err, size_t err_cap);
#endif

/* pss-bam_amd/host/mismatches.h -- pss-bam -n / -N helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_MISMATCHES_H
#define PSSBAM_MISMATCHES_H
#include <stddef.h>

/* The -n argument: the largest mismatch count a tallied read may have, 0..255 (PSSBAM_MAX_MISMATCHES) as a decimal
 * integer -- digits only: no sign, no blanks, not empty.  Returns the value, or -1 with a one-line diagnostic (no
 * newline) in err[0..err_cap). */
int pss_parse_max_mismatches(const char *arg, char *err, size_t err_cap);
/* The -N argument: the largest mismatch count that gets a row of its own, 1..255, written the same way.  Returns the
 * value, or -1 with a diagnostic. */
int pss_parse_mismatch_hist(const char *arg, char *err, size_t err_cap);
#endif

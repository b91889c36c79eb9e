/* pss-bam_amd/host/length_hist.h -- pss-bam -H helper (exported from libpssbam_host.so). */
#ifndef PSSBAM_LENGTH_HIST_H
#define PSSBAM_LENGTH_HIST_H
#include <stddef.h>

/* The -H argument: the largest length that gets a row of its own, 1..65535 (PSSBAM_MAX_HIST_LENGTH) as a decimal
 * integer -- digits only: no sign, no blanks, not empty.  Returns the value, or -1 with a one-line diagnostic (no
 * newline) in err[0..err_cap). */
int pss_parse_length_hist(const char *arg, char *err, size_t err_cap);
#endif

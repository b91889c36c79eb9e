/* pss-bam_amd/host/base_quality.h -- pss-bam -Q helper (exported from libpssbam_host.so). */
#ifndef PSSBAM_BASE_QUALITY_H
#define PSSBAM_BASE_QUALITY_H
#include <stddef.h>

/* The -Q argument: a Phred value in 0..93 (PSSBAM_MAX_BASE_QUALITY) as a decimal integer -- digits only: no sign,
 * no blanks, not empty.  Returns the value, or -1 with a one-line diagnostic (no newline) in err[0..err_cap). */
int pss_parse_min_base_quality(const char *arg, char *err, size_t err_cap);
#endif

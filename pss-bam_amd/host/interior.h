/* pss-bam_amd/host/interior.h -- pss-bam -W helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_INTERIOR_H
#define PSSBAM_INTERIOR_H
#include <stddef.h>
#include <stdint.h>

/* The -W argument: the margin d that is left out at both ends of every read, 0..65535 (PSSBAM_MAX_INTERIOR_MARGIN) as a
 * decimal integer -- digits only: no sign, no blanks, not empty.  Returns the value, or -1 with a one-line diagnostic (no
 * newline) in err[0..err_cap). */
int pss_parse_interior_margin(const char *arg, char *err, size_t err_cap);
/* The twelve substitution rates of one 4 x 4 table (cell = 4 * read base + reference base, A C G T), in the order of a row of
 * the rates file (AC AG AT CA CG CT GA GC GT TA TC TG): count / column total of the reference base, by the rule of a row of
 * that file (pss_sub_rates) -- all twelve are zero when the A, C, G or T column is empty. */
void pss_interior_rates(const uint64_t table[16], double rates[12]);
#endif

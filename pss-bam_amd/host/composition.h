/* pss-bam_amd/host/composition.h -- pss-bam -P helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_COMPOSITION_H
#define PSSBAM_COMPOSITION_H
#include <stddef.h>
#include <stdint.h>

/* The -P argument: the width w of the window on either side of a read end, 1..30 (PSSBAM_MAX_COMPOSITION) as a decimal
 * integer -- digits only: no sign, no blanks, not empty.  Returns the value, or -1 with a one-line diagnostic (no newline)
 * in err[0..err_cap). */
int pss_parse_composition_width(const char *arg, char *err, size_t err_cap);
/* The four base fractions of one row {A, C, G, T, other} of the composition table: count / (A + C + G + T), all four zero
 * when that sum is zero.  "other" is left out of the denominator. */
void pss_composition_fractions(const uint64_t row[5], double frac[4]);
#endif

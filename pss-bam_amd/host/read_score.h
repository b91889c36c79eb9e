/* pss-bam_amd/host/read_score.h -- pss-bam -y / -Y helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_READ_SCORE_H
#define PSSBAM_READ_SCORE_H
#include <stddef.h>
#include <stdint.h>

#define PSS_PMD_DIST 32      /* distance rows of the table pss-bam passes to the engine */
#define PSS_PMD_QUAL 64      /* quality columns */
#define PSS_PMD_HIST_HALF 32 /* -Y: 64 rows, whole nats -32 .. 31 */
#define PSS_PMD_HIST_SHIFT 8 /* -Y: a row is 256 units = one nat */

/* The post-mortem-damage weights of a double-stranded library, out[kind][z][q] in units of 1/256 nat: the log-likelihood ratio
 * "ancient" against "modern" of Skoglund et al. 2014 with its default parameters.  With eps = 10^(-q/10) / 3, pi = 0.001 and
 * P(D) = (1-pi)(1-eps)(1-D) + (1-pi) eps D + pi eps (1-D) the probability of a match at damage rate D, D_a(z) = 0.3 * 0.7^z + 0.01
 * at 0-based distance z from the read end (rows 0..31; the engine freezes larger distances at the last row) and D_m = 0.001:
 * kinds 0 and 2 (C read as C by distance from the 5' end, G read as G by distance from the 3' end) hold
 * llround(256 ln(P(D_a) / P(D_m))), kinds 1 and 3 (C read as T, G read as A) llround(256 ln((1 - P(D_a)) / (1 - P(D_m)))).
 * Every entry lies within +-2047. */
void pss_pmd_weights(int16_t *out /*[4][PSS_PMD_DIST][PSS_PMD_QUAL]*/);

/* The -y argument t, a decimal number: an optional '-', digits, and optionally a point with one to three digits behind it --
 * no other sign, no exponent, no blanks, not empty, below 8000000 in size.  Stores ceil(256 t), the smallest score of a tallied
 * read, worked out in integers, and returns 0; or returns -1 with a one-line diagnostic (no newline) in err[0..err_cap). */
int pss_parse_min_score(const char *arg, int32_t *min_score, char *err, size_t err_cap);
#endif

/*
 * pss-bam_amd/host/read_score.c -- pss-bam -y / -Y: the post-mortem-damage weight table and the score threshold.
 */
#include "read_score.h"

#include <math.h>
#include <stdio.h>

static double match_prob(double damage, double eps)
{
    const double pi = 0.001;
    return (1.0 - pi) * (1.0 - eps) * (1.0 - damage) + (1.0 - pi) * eps * damage + pi * eps * (1.0 - damage);
}

void pss_pmd_weights(int16_t *out)
{
    const double d_modern = 0.001;
    for (int z = 0; z < PSS_PMD_DIST; z++) {
        const double d_ancient = 0.3 * pow(0.7, (double)z) + 0.01;
        for (int q = 0; q < PSS_PMD_QUAL; q++) {
            const double eps = pow(10.0, -(double)q / 10.0) / 3.0;
            const double pa = match_prob(d_ancient, eps), pm = match_prob(d_modern, eps);
            const int16_t match = (int16_t)llround(256.0 * log(pa / pm));
            const int16_t mismatch = (int16_t)llround(256.0 * log((1.0 - pa) / (1.0 - pm)));
            for (int kind = 0; kind < 4; kind++)
                out[((size_t)kind * PSS_PMD_DIST + (size_t)z) * PSS_PMD_QUAL + (size_t)q] = (kind & 1) ? mismatch : match;
        }
    }
}

int pss_parse_min_score(const char *arg, int32_t *min_score, char *err, size_t err_cap)
{
    static const char *form = "a decimal number with at most three digits behind the point, such as 3, -0.5 or 2.125";
    if (!arg || !*arg) {
        snprintf(err, err_cap, "-y needs the smallest score of a tallied read (%s)", form);
        return -1;
    }
    const char *q = arg;
    const int negative = *q == '-';
    if (negative) q++;
    long long whole = 0, frac = 0;
    int n_whole = 0, n_frac = 0;
    for (; *q >= '0' && *q <= '9'; q++, n_whole++) {
        whole = whole * 10 + (*q - '0');
        if (whole >= 8000000) {
            snprintf(err, err_cap, "-y: the score must be below 8000000 in size");
            return -1;
        }
    }
    if (*q == '.') {
        for (q++; *q >= '0' && *q <= '9' && n_frac < 4; q++, n_frac++) frac = frac * 10 + (*q - '0');
        if (n_frac == 0 || n_frac > 3) {
            snprintf(err, err_cap, "-y: the score is not %s", form);
            return -1;
        }
        for (int k = n_frac; k < 3; k++) frac *= 10;
    }
    if (n_whole == 0 || *q != '\0') {
        snprintf(err, err_cap, "-y: the score is not %s", form);
        return -1;
    }
    const long long thousandths = whole * 1000 + frac;   /* |t| * 1000 */
    /* ceil(256 t): upwards for a positive t, towards zero for a negative one */
    *min_score = negative ? (int32_t) - (256 * thousandths / 1000) : (int32_t)((256 * thousandths + 999) / 1000);
    return 0;
}

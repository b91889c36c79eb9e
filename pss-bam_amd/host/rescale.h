/* pss-bam_amd/host/rescale.h -- quality-rescale helpers (exported from libpssbam_host.so): the rates file of an earlier run becomes
 * the table csrc/rescale_kernels.h applies to a record (hostcheck -k). */
#ifndef PSSBAM_RESCALE_H
#define PSSBAM_RESCALE_H
#include <stddef.h>
#include <stdint.h>

#define PSS_RESCALE_DS 1         /* PSSBAM_RS_DS of csrc/rescale_kernels.h */
#define PSS_RESCALE_SS 2         /* PSSBAM_RS_SS */
#define PSS_RESCALE_MAX_ROWS 64  /* PSSBAM_RS_MAX_ROWS */
#define PSS_RESCALE_QUALS 94     /* PSSBAM_RS_QUALS */

typedef struct pss_rescale {
    int mode;                    /* PSS_RESCALE_DS / _SS */
    uint32_t file_rows;          /* R: the rows of each of the file's two tables */
    uint32_t rows;               /* min(R, 64): the rows of everything below */
    double baseline[2];          /* b5, b3 */
    double rate[2][PSS_RESCALE_MAX_ROWS], damage[2][PSS_RESCALE_MAX_ROWS];   /* [0]: 5' end, [1]: 3' end */
    uint8_t table[2 * PSS_RESCALE_MAX_ROWS * PSS_RESCALE_QUALS];             /* [2][rows][94], packed by `rows` */
} pss_rescale;

/* Reads `path`, a <prefix>.pss.rates.txt as pss_write_rates writes it: '#' lines and blank lines apart, a row is its position and
 * twelve rates (AC AG AT CA CG CT GA GC GT TA TC TG), each in [0, 1]; the rows in front of the first '#' line that follows a row are
 * the forward table, positions 0, 1, ... ascending, the ones behind it the reverse table, descending to 0.  rate5[i] is column TC of
 * forward row i; rate3[i] column AG (DS) or TC (SS) of reverse row i.  baseline: in [0, 1), used for both ends; negative: none is
 * given, and each end's is the mean of its column over rows R/2 .. R-1 of all R rows.  damage d = rate > b && rate > 0 ? 1 - b / rate
 * : 0, and table[end][i][q] = d == 0 ? q : min(q, floor(-10 log10(1 - (1 - 10^(-q/10)) (1 - d)) + 0.5)), all in double precision.
 * Returns 0, or -1 with a one-line diagnostic (no newline) in err[0..err_cap): a file that cannot be read, a malformed line (the
 * message names file and line), two tables of unequal row counts, no rows, a baseline of 1 or more. */
int pss_rescale_table(const char *path, int mode, double baseline, pss_rescale *out, char *err, size_t err_cap);

/* The -k argument, <ds|ss>,<rates file>[,<baseline>]: the last comma-separated piece is the baseline when it reads as a number.
 * *path_out (may be NULL) receives a malloc'ed copy of the file's name.  Returns as pss_rescale_table. */
int pss_parse_rescale(const char *arg, pss_rescale *out, char **path_out, char *err, size_t err_cap);
#endif

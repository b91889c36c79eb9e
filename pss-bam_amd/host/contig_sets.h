/* pss-bam_amd/host/contig_sets.h -- pss-bam -C helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_CONTIG_SETS_H
#define PSSBAM_CONTIG_SETS_H
#include <stddef.h>
#include <stdint.h>

/* A -C map file's text (text[0..len)).  Each line is "<contig name>" or "<contig name><blanks><label>" (blanks =
 * spaces / tabs; the label defaults to the name); blank lines and lines whose first byte is '#' are skipped, a
 * CR before the LF is dropped.  Labels are numbered in order of first appearance.  A name repeated under the
 * same label counts once; under two labels it is an error naming both lines.  Returns the number of names
 * (*names, (*set_of)[i] = label index of name i) and puts the labels in *labels / *n_labels (everything
 * malloc'ed: pss_free_contig_sets), or -1 with a one-line diagnostic (no newline) in err[0..err_cap): no label
 * at all, more than PSSBAM_MAX_CONTIG_SETS labels, a name under two labels, a NUL byte, out of memory. */
int pss_parse_contig_sets(const char *text, size_t len, char ***names, int32_t **set_of, char ***labels, int *n_labels,
                          char *err, size_t err_cap);
void pss_free_contig_sets(char **names, int n_names, int32_t *set_of, char **labels, int n_labels);
#endif

/* pss-bam_amd/host/read_groups.h -- pss-bam -G helpers (exported from libpssbam_host.so). */
#ifndef PSSBAM_READ_GROUPS_H
#define PSSBAM_READ_GROUPS_H
#include <stddef.h>

/* The ID: values of the @RG lines of SAM header text (text[0..len), stops at a NUL), in header order; a
 * repeated ID counts once (its first line), a line without an ID: field (or with an empty one) is skipped; the
 * ID: field may be any field of the line, lines may end in CRLF.  *ids is malloc'ed (pss_free_read_groups).
 * Returns the number of IDs, or -1 when out of memory. */
int pss_parse_read_groups(const char *text, size_t len, char ***ids);
void pss_free_read_groups(char **ids, int n);
/* The ID as it appears in an output file name: every byte outside [A-Za-z0-9_-] becomes %XX (uppercase hex).
 * Writes at most cap-1 bytes + NUL; returns the full length (without the NUL). */
size_t pss_rg_file_tag(const char *id, char *out, size_t cap);
#endif

/* pss-bam_amd/host/duplicates.h -- the report of -d (duplicate flagging, include/pssbam_hip.h: pssbam_engine_set_duplicates). */
#ifndef PSSBAM_DUPLICATES_H
#define PSSBAM_DUPLICATES_H

#include <stdint.h>

#define PSS_DUP_HIST_MAX 255   /* group sizes with a row of their own; the last row is every larger group */

/* Writes <out_prefix>.<tool>.duplicates.txt (tool = "pss" or "fragkon"): the three totals of pssbam_engine_finish_duplicates,
 * the duplicate fraction (flagged / eligible, 0 without eligible records) and the group-size histogram -- "size<TAB>groups" for
 * sizes 1..hist_max, then ">hist_max".  hist has hist_max + 2 entries, as the engine returns them.  Returns 0, or 1 after a
 * message on stderr. */
int pss_write_duplicates(const char *fasta_fn, const char *bam_fn, const char *out_prefix, const char *tool, const uint64_t totals[3],
                         const uint64_t *hist, int hist_max);

#endif

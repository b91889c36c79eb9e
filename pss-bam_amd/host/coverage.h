/* pss-bam_amd/host/coverage.h -- the reports of -c and -b (depth of coverage of the tallied reads, include/pssbam_hip.h:
 * pssbam_engine_set_coverage). */
#ifndef PSSBAM_COVERAGE_H
#define PSSBAM_COVERAGE_H

#include <stdint.h>

#define PSS_COV_HIST_MAX 255   /* depths with a row of their own; the last row is every larger depth */

/* Writes <out_prefix>.pss.coverage.txt.  The n references are those of the input's header, in its order; held[i] != 0 marks the ones
 * the FASTA holds, and only those get a line: "contig length covered_bases breadth depth_sum mean_depth max_depth" (tab-separated;
 * breadth = covered / length and mean_depth = depth_sum / length with six decimals, 0 for an empty contig), then a "total" line over
 * them, then the depth histogram -- "depth<TAB>positions" for 0..hist_max, then ">hist_max".  per_contig has n x {covered, depth_sum,
 * max_depth} and hist hist_max + 2 entries, as pssbam_engine_finish_coverage returns them.  Returns 0, or 1 after a message on
 * stderr. */
int pss_write_coverage(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int n, const char *const *names, const uint8_t *held,
                       const uint64_t *lengths, const uint64_t *per_contig, const uint64_t *hist, int hist_max);

/* Writes the runs of pssbam_engine_finish_coverage_runs as a bedGraph, "contig<TAB>start<TAB>end<TAB>depth", 0-based and half-open,
 * in the order given (ref[i] indexes names, n of them).  The file is written as <path>.tmp and takes its name when it is complete;
 * a failure leaves neither.  Returns 0, or 1 after a message on stderr. */
int pss_write_coverage_bedgraph(const char *path, int n, const char *const *names, uint64_t n_runs, const int32_t *ref, const uint32_t *start,
                                const uint32_t *end, const uint32_t *depth);

#endif

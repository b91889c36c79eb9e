/* pss-bam_amd/host/windows.h -- the reports of -w (fixed windows over the depth of coverage of the tallied reads, include/pssbam_hip.h:
 * pssbam_engine_finish_coverage_windows). */
#ifndef PSSBAM_WINDOWS_H
#define PSSBAM_WINDOWS_H

#include <stdint.h>

#define PSS_WINDOW_MIN 16u
#define PSS_WINDOW_MAX (1u << 30)
#define PSS_GC_BINS 101   /* GC percentages 0..100 */

/* "-w <size>": a whole number in PSS_WINDOW_MIN..PSS_WINDOW_MAX and nothing else.  Returns 0 and the size, or 1. */
int pss_parse_window(const char *arg, uint32_t *window);

/* The GC-bias table over n windows.  A window is used when end - start == window and 2 * acgt >= window; its bin is
 * (200 * gc + acgt) / (2 * acgt) in integer division: the GC percentage of its A/C/G/T letters, rounded half up.  A window with gc > acgt, which the engine never
 * gives, is left out too: its bin would lie beyond 100.  bin_windows and
 * bin_depth_sum have PSS_GC_BINS entries: the used windows of each bin and their summed depth.  Returns the number of used windows. */
uint64_t pss_gcbias_rows(uint32_t window, uint64_t n, const uint32_t *start, const uint32_t *end, const uint32_t *acgt, const uint32_t *gc,
                         const uint64_t *depth_sum, uint64_t *bin_windows, uint64_t *bin_depth_sum);

/* Writes <out_prefix>.pss.windows.txt and <out_prefix>.pss.gcbias.txt from the n windows of pssbam_engine_finish_coverage_windows, in
 * the order given (ref[i] indexes names, n_names of them).
 *   windows: comment lines (what it is, FASTA, BAM, window, windows), the column line, then per window, tab-separated, "contig start
 *     end acgt gc gc_fraction covered depth_sum mean_depth"; gc_fraction = gc / acgt with six decimals, NA when acgt is 0;
 *     mean_depth = depth_sum / (end - start) with six decimals.
 *   gcbias: comment lines (what it is, FASTA, BAM, window, windows, used windows, mean depth of the used windows), the column line,
 *     then PSS_GC_BINS rows "gc_percent windows positions depth_sum mean_depth relative_depth"; positions = windows * window,
 *     mean_depth = depth_sum / positions, relative_depth = mean_depth / the mean depth of the used windows; six decimals, 0 where a
 *     denominator is 0.
 * Each file is written as <name>.tmp and takes its name when both are complete; a failure leaves neither.  Returns 0, or 1 after a
 * message on stderr. */
int pss_write_windows(const char *fasta_fn, const char *bam_fn, const char *out_prefix, uint32_t window, int n_names, const char *const *names,
                      uint64_t n, const int32_t *ref, const uint32_t *start, const uint32_t *end, const uint32_t *acgt, const uint32_t *gc,
                      const uint32_t *covered, const uint64_t *depth_sum);

#endif

/* pss-bam_amd/host/frontend.h -- what the two command-line front ends share: open the
 * alignment input, drive one engine per GPU over its record batches, gather the tables. */
#ifndef PSSBAM_FRONTEND_H
#define PSSBAM_FRONTEND_H

#include <stdint.h>

#include "fasta-genome-io.h"
#include "pssbam_hip.h"
#include "alleles.h"
#include "coverage.h"
#include "duplicates.h"
#include "regions.h"

typedef struct run_result {
    unsigned long *fwd, *rev; /* (region_len+2)*16 each, or NULL */
    uint64_t *k5, *k3;        /* 4^klen each, or NULL            */
    uint64_t stats[PSSBAM_ST_N];
    double inflate_s, total_s;
    int n_gpus;
    /* pss-bam -G / -S / -C: the tables of each plane of the engine, (region_len+2)*16 per plane; plane k is the
     * header's k-th @RG ID (frontend_opts.group_by_rg, group_ids[k]), length bin k (frontend_opts.length_edges, group_ids
     * NULL) or the k-th label of frontend_opts.contig_sets (group_ids NULL); pss-bam -J: replicate k (frontend_opts.replicates,
     * group_ids NULL) */
    int n_planes;
    char **group_ids;
    unsigned long *plane_fwd, *plane_rev;
    /* fragkon -G / -S / -C (a PSSBAM_TALLY_KMER engine): the planes' k-mer tables instead, 4^klen per plane */
    uint64_t *plane_k5, *plane_k3;
    /* pss-bam -H (frontend_opts.length_hist): the fragment-length histogram of the reads added to the forward / reverse
     * table, hist_max + 2 rows each (row hist_max + 1: every longer read), or NULL */
    int hist_max;
    uint64_t *hist_fwd, *hist_rev;
    /* pss-bam -N (frontend_opts.mismatch_hist): the mismatch histogram of the reads added to the forward / reverse table,
     * mism_max + 2 rows each (row mism_max + 1: every larger count), or NULL */
    int mism_max;
    uint64_t *mism_fwd, *mism_rev;
    /* pss-bam -W (frontend_opts.interior): the interior table and the number of reads that have an interior (has_interior: filled) */
    int has_interior;
    uint64_t interior[16], interior_reads;
    /* pss-bam -P (frontend_opts.composition): the two blocks of the composition table, 2 * composition_width rows of five counts
     * each (malloc'ed), or NULL */
    int composition_width;
    uint64_t *comp5, *comp3;
    /* pss-bam -Y (frontend_opts.read_score with a histogram): the score histogram of the reads added to the forward / reverse
     * table, 2 * score_half rows each, or NULL */
    int score_half;
    uint64_t *score_fwd, *score_rev;
    /* pss-bam -X (frontend_opts.site_context): the in-context tables IN, (region_len+2)*16 each with rows 0/1 as fwd / rev,
     * or NULL */
    unsigned long *site_fwd, *site_rev;
    /* pss-bam -E (frontend_opts.end_depth): the conditional tables COND, (region_len+2)*16 each, or NULL, and reads[4] */
    unsigned long *end_fwd, *end_rev;
    uint64_t end_reads[4];
    /* pss-bam -A (frontend_opts.per_contig): the tables of every reference that holds something, in header order (the refID -1
     * records last, under the name "*"): n_contigs names and tables of (region_len+2)*16 each */
    int n_contigs;
    char **contig_names;
    unsigned long *contig_fwd, *contig_rev;
    /* -d (frontend_opts.duplicates; has_duplicates: filled): {eligible, distinct, flagged} and the group-size histogram,
     * PSS_DUP_HIST_MAX + 2 entries (duplicates.h) */
    int has_duplicates;
    uint64_t dup_totals[3], dup_hist[PSS_DUP_HIST_MAX + 2];
    /* -c / -b (frontend_opts.coverage / .coverage_bedgraph; has_coverage: filled): the cov_n references of the input, in header
     * order -- name, whether the FASTA holds it, its length there, {covered, depth_sum, max_depth} -- the depth histogram,
     * PSS_COV_HIST_MAX + 2 entries (coverage.h), and, for -b, the cov_n_runs runs (pssbam_engine_finish_coverage_runs) */
    int has_coverage, cov_n;
    char **cov_names;
    uint8_t *cov_held;
    uint64_t *cov_lengths, *cov_per_contig, cov_hist[PSS_COV_HIST_MAX + 2], cov_n_runs;
    int32_t *cov_run_ref;
    uint32_t *cov_run_start, *cov_run_end, *cov_run_depth;
    /* -w (frontend_opts.coverage_window; filled with has_coverage): the win_n windows of pssbam_engine_finish_coverage_windows, by
     * reference (an index into cov_names) and start */
    uint64_t win_n, *win_depth_sum;
    int32_t *win_ref;
    uint32_t *win_start, *win_end, *win_acgt, *win_gc, *win_covered;
    /* -a (frontend_opts.sites; has_alleles: filled): the allele_n_names references of the input, in header order, and what
     * pssbam_engine_finish_sites gave: the allele_n resolved sites' reference index, 0-based position, reference letter and ten
     * counters each, and the four totals */
    int has_alleles, allele_n_names;
    char **allele_names;
    uint64_t allele_n, allele_totals[4];
    int32_t *allele_ref;
    uint32_t *allele_pos, *allele_counts;
    uint8_t *allele_base;
} run_result;

/* -y / -Y: the weight table [4][n_dist][n_qual], the filter (use_filter: only reads with a score of at least min_score are
 * tallied) and the histogram (hist_half = 0: none) */
typedef struct frontend_score {
    const int16_t *weights;
    int n_dist, n_qual, use_filter, min_score, hist_half, hist_shift;
} frontend_score;

/* -C: the contig -> set map (contig_sets.h) */
typedef struct frontend_contig_map {
    int n_names, n_labels;
    char **names, **labels;
    int32_t *set_of;
} frontend_contig_map;

/* The tally options of a run: main() fills frontend_opts before frontend_warmup_start and leaves it alone from then on (the
 * helper thread and run_tally() read it; the pointers are kept).  Every engine of the run gets them (apply_options in
 * frontend.c). */
typedef struct frontend_options {
    /* pss-bam -G: every engine gets the input header's @RG IDs (pssbam_engine_set_read_groups) and run_tally()
     * returns one pair of tables per ID beside the totals. */
    int group_by_rg;
    /* pss-bam -S: the edges of the length bins (n_length_edges = 0: none); every engine gets them
     * (pssbam_engine_set_length_bins) and run_tally() returns one pair of tables per bin. */
    int n_length_edges;
    uint32_t length_edges[PSSBAM_MAX_LENGTH_BINS - 1];
    /* pss-bam -C: the contig -> set map (NULL: none); every engine gets it (pssbam_engine_set_contig_sets) and run_tally()
     * returns one pair of tables per label, and warns on stderr about a label none of whose contigs is both in the input's
     * references and in the genome. */
    const frontend_contig_map *contig_sets;
    /* pss-bam -Q: the minimum base quality (0: off); every engine gets it (pssbam_engine_set_min_base_quality). */
    int min_base_quality;
    /* pss-bam -H: the limit of the fragment-length histogram (0: off); every engine gets it
     * (pssbam_engine_set_length_histogram) and run_tally() returns the two arrays. */
    int length_hist;
    /* pss-bam -N / -n / -V: the limit of the mismatch histogram (0: off), the largest mismatch count of a tallied read (-1: no
     * filter) and whether only transversions count; every engine gets them (pssbam_engine_set_mismatches) and run_tally()
     * returns the two arrays of the histogram. */
    int mismatch_hist, max_mismatches, mismatch_tv;
    /* pss-bam -W: the interior margin (-1: off); every engine gets it (pssbam_engine_set_interior) and run_tally() returns the
     * table and its read count. */
    int interior;
    /* pss-bam -P: the width of the composition table (0: off); every engine gets it (pssbam_engine_set_composition) and
     * run_tally() returns the two blocks. */
    int composition;
    /* pss-bam -y / -Y: the read score (NULL: off); every engine gets it (pssbam_engine_set_read_score) and run_tally() returns
     * the two arrays of the histogram. */
    const frontend_score *read_score;
    /* pss-bam -X: the site context (PSSBAM_SITE_*; PSSBAM_SITE_NONE: off); every engine gets it
     * (pssbam_engine_set_site_context) and run_tally() returns the in-context pair. */
    int site_context;
    /* pss-bam -E: the end condition (depth 0: off) and its two cells; every engine gets them
     * (pssbam_engine_set_end_condition) and run_tally() returns the conditional pair and reads[4]. */
    int end_depth, end_cell5, end_cell3;
    /* pss-bam -I: non-zero = every engine tallies clipped and gapped reads by their anchored ends
     * (pssbam_engine_set_gapped_reads). */
    int gapped_reads;
    /* pss-bam -A: non-zero = every engine keeps a pair of tables per reference (pssbam_engine_set_per_contig) and run_tally()
     * returns those that hold something. */
    int per_contig;
    /* pss-bam -J: the number of read-name replicates (0: off); every engine gets it (pssbam_engine_set_replicates) and
     * run_tally() returns one pair of tables per replicate in plane_fwd / plane_rev (n_planes = the count, group_ids NULL),
     * summed over the GPUs with the rest of the counter block. */
    int replicates;
    /* -T: the intervals of the BED file (regions.h; NULL: none); every engine gets them (pssbam_engine_set_regions), on
     * every input path -- the filter lives in the engine. */
    const pss_regions *regions;
    /* pss-bam -O / -z: the BAM that receives the records added to a table (NULL: none) and its compression level; the run's
     * one engine gets a record sink (pssbam_engine_set_record_sink) that appends to a bam_writer.  run_tally() closes the file
     * -- it takes its name only then -- before it returns, and removes it when the run fails.  BAM input, one GPU. */
    const char *out_bam;
    int out_level;
    /* pss-bam -Z: the engine deflates the kept records into BGZF blocks itself (pssbam_engine_set_block_sink) and the writer
     * only writes them (bam_writer_append_blocks); the header still goes through the writer's own blocks */
    int out_deflate;
    /* pss-bam -K: the end mask of the -O file (PSSBAM_END_MASK_*; PSSBAM_END_MASK_OFF: none) and the widths of its 5' and 3'
     * regions; the run's one engine gets them beside its sink (pssbam_engine_set_end_mask) */
    int out_mask_mode;
    uint32_t out_mask_n5, out_mask_n3;
    /* -d: non-zero = the run's one engine flags the duplicates in front of its tally (pssbam_engine_set_duplicates) and
     * run_tally() returns the totals and the group-size histogram.  One GPU: duplicates are defined by the input order. */
    int duplicates;
    /* pss-bam -c / -b: coverage != 0 = the summary is wanted, coverage_bedgraph != NULL = the runs are; with either, the run's one
     * engine keeps the depth of coverage of the reads it adds to a table (pssbam_engine_set_coverage, with the sum of the header's
     * LN values as its hint) and run_tally() returns the per-contig figures and the histogram, and for -b the runs.  One GPU. */
    int coverage;
    const char *coverage_bedgraph;
    /* pss-bam -w: non-zero = the window size; switches the same array on, and run_tally() returns the windows
     * (pssbam_engine_finish_coverage_windows).  One GPU. */
    uint32_t coverage_window;
    /* pss-bam -a / -t: the sites of the sites file (alleles.h; NULL: none) and the trim; the run's one engine counts the bases the
     * reads it adds to a table show there (pssbam_engine_set_sites) and run_tally() returns the counts.  One GPU. */
    const pss_sites *sites;
    uint32_t site_trim;
} frontend_options;
extern frontend_options frontend_opts;   /* everything off */

/* Streams every alignment of `aln_path` (BGZF BAM, or SAM text plain/gzip) through engines built from `cfg` on
 * n_gpus devices (batches dealt round-robin), sums the counter blocks onto device 0 with
 * RCCL when n_gpus > 1, and returns the tables in *res (caller frees with run_result_free).
 * Returns 0, or -1 after printing a diagnostic to stderr. */
int run_tally(const pssbam_config *cfg, Genome *genome, const char *aln_path, int n_gpus, run_result *res);

/* The command-line tools end right after their report is written: with this set (they set it
 * unless $PSSBAM_CLEAN_EXIT is), run_tally() leaves engines, pinned slots and the mapped input
 * to process exit instead of releasing ~4 GB piece by piece (0.12 s of a 0.7 s command), and
 * front_end_exit() ends the process without running destructors. */
/* Start-up work that overlaps the caller's FASTA load (returns at once).  If aln_path is a BGZF BAM the
 * device feed takes, a helper thread brings the HIP runtime up, creates the engines from `cfg` and feeds the
 * compressed file to them right away -- inflate, CRC-32 and record index need no genome; run_tally() (same
 * cfg, same path) posts the Genome when the caller has it and collects the result.  Otherwise (SAM text, host
 * inflate, cfg == NULL) the helper only warms the runtime up and page-locks the host reader's slots.
 * fasta_path (may be NULL) only sizes the device memory left alone for the genome.  aln_path may be NULL. */
void frontend_warmup_start(const pssbam_config *cfg, const char *aln_path, const char *fasta_path);

/* First statement of a front end's main(): forks the worker that runs the rest of main(); the process the caller
 * started returns the worker's exit status as soon as front_end_exit() sends it, without waiting for the worker's
 * teardown (frontend.c; PSSBAM_DETACH_EXIT=0 or a non-empty LD_PRELOAD: no fork). */
void frontend_detach_start(void);
int frontend_detached(void); /* 1 in a worker whose caller will be released by front_end_exit() */

extern int frontend_fast_exit;
void front_end_exit(int status);
/* The end of a front end whose run has failed, after its message, while the helper thread of frontend_warmup_start() may still be
 * inside the HIP runtime's start-up: flushes stdio and ends the process without running exit handlers or destructors -- exit()
 * would take the runtime's own state apart under that thread, which now and then ended in SIGSEGV or abort() instead of `status`. */
void front_end_fail(int status);
void run_result_free(run_result *res);
double frontend_now_s(void); /* CLOCK_MONOTONIC seconds */
double frontend_process_age_s(void); /* seconds since the process was created (10 ms resolution), -1 if unknown */
int env_gpu_count(void); /* PSSBAM_NGPU, default 1, clamped to the devices present */
#endif

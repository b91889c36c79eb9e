/* pss-bam_amd/host/report.h -- report writers of the two front ends (byte-exact parity surface). */
#ifndef PSSBAM_REPORT_H
#define PSSBAM_REPORT_H
#include <stdint.h>
#include <stdio.h>

/* rates[i*12 + j], j = AC AG AT CA CG CT GA GC GT TA TC TG; counts = (region_len+2)*16 */
void pss_sub_rates(int region_len, const unsigned long *counts, double *rates);
int pss_write_counts(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len,
                     const unsigned long *fwd, const unsigned long *rev);
int pss_write_rates(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len,
                    const double *fwd_rates, const double *rev_rates);
/* pss-bam -J: <out_prefix>.pss.rates.se.txt in the layout of the rates file -- the same "###" lines (OUT: names this file; the
 * two captions read "### jackknife standard errors of the forward / reverse read substitution rates, K = <k> read-name
 * replicates"), the forward rows 0 .. N-1, two blank lines, the reverse rows N-1 .. 0, every value "%.5e".  fwd_se / rev_se
 * hold region_len * 12 values in pss_sub_rates' order (replicates.h: pss_jackknife_se).  Returns 0, or 1 after a diagnostic. */
int pss_write_rates_se(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len, int k,
                       const double *fwd_se, const double *rev_se);
/* One labelled pair of files, <out_prefix>.<tag>.pss.counts.txt and .rates.txt, through the two writers above (what
 * -G / -S / -C write per plane and -X per context); `tag` is already file-name encoded.  Returns 0, or 1 after a
 * diagnostic. */
int pss_write_labelled(const char *fasta_fn, const char *bam_fn, const char *out_prefix, const char *tag, int region_len,
                       const unsigned long *fwd, const unsigned long *rev);
/* pss-bam -A: <out_prefix>.pss.contigs.txt -- the four "###" lines that open a counts file (version, FASTA, BAM, OUT: this
 * file), the line "### CONTIG TABLE POS AA AC ... TT", then for each of the n contigs, in the order given, the body lines
 * of its counts file, each behind "<name><TAB>fwd<TAB>" or "<name><TAB>rev<TAB>": the forward rows -2 .. N-1, the reverse
 * rows N-1 .. 0, 1, 2.  fwd / rev hold n tables of (region_len + 2) * 16 counts.  Returns 0, or 1 after a diagnostic. */
int pss_write_contigs(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int region_len, int n,
                      const char *const *names, const unsigned long *fwd, const unsigned long *rev);
/* pss-bam -E: parses "<ss|ds>[,<d>]" -- ss: C->T at both ends (cell5 = cell3 = 13, column TC), ds: C->T at the 5' end
 * and G->A at the 3' end (cell5 = 13, cell3 = 2, column AG); d = 1..PSSBAM_MAX_END_DEPTH, default 1.  Returns 0, or -1
 * with a one-line message in err. */
int pss_parse_end_condition(const char *arg, int *depth, int *cell5, int *cell3, char *err, size_t err_len);
/* pss-bam -E: <out_prefix>.cond.pss.reads.txt -- four "<name><TAB><value>" lines: the unpaired reads added to the tables,
 * the 5'-marked, the 3'-marked and the both-marked ones among them.  Returns 0, or 1 after a diagnostic. */
int pss_write_end_reads(const char *out_prefix, const uint64_t reads[4]);
/* pss-bam -H: <out_prefix>.pss.lengths.txt -- three '#' lines, the column names, then one tab-separated line
 * "<length> <fwd> <rev>" per length 0..max_len (zero rows included) and a last one labelled "><max_len>" for every
 * longer read; fwd / rev hold max_len + 2 counts.  Returns 0, or 1 after a diagnostic. */
int pss_write_lengths(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int max_len, const uint64_t *fwd,
                      const uint64_t *rev);
/* pss-bam -N: <out_prefix>.pss.mismatches.txt, in the layout of the lengths file -- three '#' lines (the first says whether all
 * mismatches or transversions only were counted), the column names, then one tab-separated line "<mismatches> <fwd> <rev>"
 * per count 0..max_mm (zero rows included) and a last one labelled "><max_mm>" for every larger count; fwd / rev hold
 * max_mm + 2 counts.  Returns 0, or 1 after a diagnostic. */
int pss_write_mismatches(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int max_mm, int transversions_only,
                         const uint64_t *fwd, const uint64_t *rev);
/* pss-bam -W: <out_prefix>.pss.interior.txt -- a '#' line that states the margin (and the minimum base quality when min_bq > 0) and
 * two with the input names, the column names of the counts file and one row of the 16 counts labelled with the margin, printed as
 * a row of the counts file; the column names of the rates file and one row of the 12 rates (pss_interior_rates), printed as a row
 * of the rates file; then "reads\t<reads>" and "bases\t<sum of the 16 counts>".  Returns 0, or 1 after a diagnostic. */
int pss_write_interior(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int margin, int min_bq, const uint64_t table[16],
                       uint64_t reads);
/* pss-bam -P: <out_prefix>.pss.composition.txt -- a '#' line that states the width and two with the input names, the column
 * names "### POS A C G T other fA fC fG fT", a "### Forward..." line and the 5' block's rows labelled -width .. -1, 0 .. width-1;
 * two blank lines; a "### Reverse..." line and the 3' block's inside rows labelled width-1 .. 0, then its outside rows labelled
 * 1 .. width (1 = the base next to the read), as the counts file orders its reverse table.  A row is the label, the five counts
 * of A C G T and other ("%lu") and the four fractions count / (A + C + G + T) ("%.5e", all zero when the sum is zero), every
 * field followed by a TAB.  c5 / c3: 2 * width rows of five counts, row j + width = offset j.  Returns 0, or 1 after a diagnostic. */
int pss_write_composition(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int width, const uint64_t *c5,
                          const uint64_t *c3);
/* pss-bam -Y: <out_prefix>.pss.pmd.txt, in the layout of the mismatches file -- three '#' lines, the column names, then one
 * tab-separated line "<score> <fwd> <rev>" per bin of the engine's score histogram (zero rows included): the first labelled
 * "<-(hist_half-1)" for every score below that many nats, then one per whole nat -(hist_half-1) .. hist_half-2 (a score is rounded
 * down), the last ">=(hist_half-1)"; fwd / rev hold 2 * hist_half counts.  Returns 0, or 1 after a diagnostic. */
int pss_write_read_scores(const char *fasta_fn, const char *bam_fn, const char *out_prefix, int hist_half, const uint64_t *fwd,
                          const uint64_t *rev);
/* k5 / k3: 4^klen 64-bit bins (clamped to UINT_MAX on output) */
int fragkon_write_table(FILE *out, const char *fasta_fn, const char *bam_fn, int klen, const uint64_t *k5,
                        const uint64_t *k3);
/* counts: 4^klen 64-bit bins (clamped to UINT_MAX on output) */
/* fragkon -G / -S / -C: one plane's table as <out_prefix>.<tag>.fragkon.txt in fragkon_write_table's format (the
 * counts stick at UINT_MAX per plane); `tag` is already file-name encoded.  Returns 0, or 1 after a diagnostic. */
int fragkon_write_plane(const char *fasta_fn, const char *bam_fn, const char *out_prefix, const char *tag, int klen,
                        const uint64_t *k5, const uint64_t *k3);
int gkc_write_table(FILE *out, int klen, const uint64_t *counts);
#endif

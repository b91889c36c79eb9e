/*
 * pss-bam_amd/host/pss_main.c -- the `pss-bam` command, MI355X edition.
 *
 * Same command line, same stderr banners, same two output files byte for byte as the
 * reference front end (/root/reference/pss-bam.c:650-805).  What changed underneath:
 *   - the BAM is read natively (BGZF inflate on host threads) instead of through a
 *     `samtools view` child and a text parser;
 *   - filtering and tallying of every alignment happen on the GPU(s) (include/pssbam_hip.h);
 *   - PSSBAM_NGPU=<n> in the environment spreads record batches over n GPUs of the node.
 * Added: -G writes, beside the tables of all reads, one pair of tables per @RG ID of the header
 * (<prefix>.<ID>.pss.*.txt, the ID file-name encoded: read_groups.h), each the same as `-R <ID>`
 * would write -- from one pass over the input instead of one run per read group.
 * Added: -S e1,...,ek writes, beside the tables of all reads, one pair of tables per fragment-length bin
 * [l, e1-1], [e1, e2-1], ..., [ek, L] (<prefix>.len<lo>-<hi>.pss.*.txt), each the same as
 * `-l <lo> -L <hi> -o <prefix>.len<lo>-<hi>` would write -- again from one pass over the input.
 * Added: -C <map file> writes, beside the tables of all reads, one pair of tables per label of the map
 * (lines "<contig name>[<blanks><label>]", contig_sets.h; <prefix>.<label>.pss.*.txt, the label file-name
 * encoded like an -G ID), each the same as a run with -F reduced to the label's contigs would write (the
 * reference skips every read whose RNAME its FASTA lacks) -- one pass instead of one run per organism, per
 * mtDNA / nuclear / X / Y split.
 * Added: -Q <q> leaves every read base whose Phred quality is below q (0..93; 0 = off) out of the tables: they
 * are the tables this command writes without -Q for the same input with those bases replaced by N.  The context
 * rows, the filters and the file names stay as they are.
 * Added: -T <bed> tallies only the reads whose alignment overlaps an interval of the BED file (plain text; contig,
 * 0-based start, end): every file written holds what this command writes without -T for the input reduced by
 * `samtools view -L <bed>`.  The file names stay as they are.
 * Added: -H <max> also writes <prefix>.pss.lengths.txt, the fragment-length histogram (the length -l / -L compare,
 * 0..max and one row for everything longer) of the reads that were added to the forward / reverse table, from the
 * same pass; the other files stay as they are.  Not with -G, -S or -C.
 * Added: -X cpg also writes <prefix>.cpg.pss.*.txt, the tables over the positions whose reference site lies in a CpG
 * dinucleotide (C followed by G, or G preceded by C, in the folded reference), and <prefix>.noncpg.pss.*.txt, the tables
 * over every other position -- what this command writes for the input with the read bases at the other kind of site
 * replaced by N -- from the same pass; the other files stay as they are.  Not with -G, -S, -C or -H.
 * Added: -E <ss|ds>[,<d>] also writes <prefix>.cond.pss.*.txt, the conditional tables: the forward table over the unpaired
 * reads that carry a G->A (ds) or C->T (ss) within the first d (default 1) positions of their 3' end, the reverse table
 * over those that carry a C->T within the first d positions of their 5' end -- what this command writes for the input
 * reduced to those reads -- and <prefix>.cond.pss.reads.txt with the four read counts, from the same pass; the other
 * files stay as they are.  Needs -r <= 30.  Not with -G, -S, -C, -H or -X.
 * Added: -I also tallies the reads whose CIGAR is not <len>M but still anchors both ends: optional hard and soft clips around a
 * core of M I D = X ops that starts and ends with a match-type op.  The two files are what this command writes without -I for
 * the input in which each such read is the record <span>M (span = the reference length of the core) whose SEQ / QUAL keep the
 * match-type run at either end of the core, with N / ! in between.  Not with -G, -S, -C, -H, -X or -E.
 * Added: -A also writes <prefix>.pss.contigs.txt: for every reference sequence of the input that holds something, in header
 * order, the rows of the counts file this command writes with -F reduced to that contig, each behind the contig's name and
 * "fwd" or "rev" (report.h) -- any number of contigs, one pass, no map file; the other files stay as they are.  The reads
 * of RNAME "*" come last, as "*".  Goes with -R, -Q and -T.  Not with -G, -S, -C, -H, -X, -E or -I.
 * Added: -n <k> tallies only the reads with at most k (0..255) mismatches against the reference over their whole length -- the
 * files are what this command writes without -n for the input without the reads beyond k; -N <M> (1..255) also writes
 * <prefix>.pss.mismatches.txt, how many of the reads added to the forward / reverse table have 0, 1, ..., M and more than M
 * mismatches, from the same pass; -V, with either, counts only transversions (deamination makes none).  A position counts
 * when read and reference base are both one of A C G T.  Needs -r <= 30.  Goes with -R, -Q and -T.  Not with -G, -S, -C, -H, -X,
 * -E, -I or -A.
 * Added: -J <K> (2..64) also writes <prefix>.pss.rates.se.txt, the delete-one-group jackknife standard error of every number in the
 * rates file, in its layout: the reads are split into K replicates by a hash of their names (mates stay together), every replicate's
 * tables come from the same pass, and the rates of the input without replicate j, j = 0 .. K-1, give the error (replicates.h).  The
 * other files stay as they are.  Goes with -R, -Q, -T, -m, -l, -L, -q, -U and -D.  Not with -G, -S, -C, -H, -X, -E, -I, -A, -n, -N or -V.
 * Added: -W <d> (0..65535) also writes <prefix>.pss.interior.txt, the 4 x 4 substitution counts and the twelve rates of the read
 * interior -- every position at least d bases from both ends of a read that is added to a table, in the read's orientation, under
 * -Q only the bases that pass it -- with the number of such reads and bases, from the same pass: the background the end rows are read
 * against.  d = 0 is the whole read.  The other files stay as they are.  Needs -r <= 30.  Goes with -R, -Q, -T, -m, -l, -L, -q, -U and
 * -D.  Not with -G, -S, -C, -H, -X, -E, -I, -A, -n, -N, -V or -J.
 * Added: -P <w> (1..30) also writes <prefix>.pss.composition.txt, the reference base composition (A C G T, other, and the four base
 * fractions) at every offset -w .. w-1 from the 5' end of the reads that are added to the forward table and from the 3' end of those
 * that are added to the reverse table, outside (negative) and inside the read, in the read's orientation, from the same pass: the
 * depurination signal next to the read against its own baseline further out.  Rows -1 and -2 are the diagonal of the counts
 * file's context rows.  The other files stay as they are.  Needs -r <= 30.  Goes with -R, -Q (no effect), -T, -m, -l, -L, -q, -U and -D.
 * Not with -G, -S, -C, -H, -X, -E, -I, -A, -n, -N, -V, -J or -W.
 * Added: -y <t> tallies only the reads whose post-mortem-damage score is at least t -- the files are what this command writes
 * without -y for the input without the other reads; -Y also writes <prefix>.pss.pmd.txt, how many of the reads added to the forward
 * / reverse table have a score of n nats, rounded down, n = -31 .. 30, and below / above, from the same pass.  The score is the
 * log-likelihood ratio "ancient" against "modern" of Skoglund et al. 2014 for a double-stranded library with its default
 * parameters, summed over the C and G sites of the read (read_score.h; under -Q only the bases that pass it), held as an integer in
 * units of 1/256 nat: -y 3 keeps the reads with a score of at least 768 units.  No number-for-number parity with another
 * implementation of the score is claimed.  Needs -r <= 30.  Goes with -R, -Q, -T, -m, -l, -L, -q, -U and -D.  Not with -G, -S, -C,
 * -H, -X, -E, -I, -A, -n, -N, -V, -J, -W or -P.
 * Added: -O <out.bam> also writes a BAM that holds exactly the alignment records that were added to the forward or the reverse
 * table of this run -- after every filter given, each mate judged on its own -- in input order and byte for byte as they are in the
 * input (unless -K), under the input's header (no @PG line), from the same pass: the file the other options' "the input without the other
 * reads" speaks of.  -Q masks bases, not reads: it changes the file only through -y.  -z <level> (0..9, default 1) is its BGZF
 * compression level.  The file is written as <out.bam>.tmp and takes its name when it is complete; a failed run leaves none.  Goes
 * with every other option.  Needs BAM input and one GPU (PSSBAM_NGPU unset or 1); must not be the file -B names.
 * Added: -Z, with -O: the file's blocks are deflated on the GPU in the same pass (the engine's block sink), not by zlib on the
 * host; the kept records are cut every 0xFF00 bytes, records crossing blocks, the header stays in blocks of its own, and the file
 * inflates to the bytes it inflates to without -Z.  Not with -z (zlib's level has no meaning there); refused without -O.
 * Added: -K <all|ds|ss>,<n5>[,<n3>], with -O: in the file's records the first n5 bases of the 5' end and the first n3 (default: n5)
 * of the 3' end of each read -- all of them (all), the T of the 5' and the A of the 3' end (ds: a double-stranded library's C->T
 * and G->A) or the T of both ends (ss), in the read's orientation -- are N with quality 0, from the same pass (the engine's end
 * mask, include/pssbam_hip.h); everything else of the file is what it is without -K, and so is every other file: the tables are
 * those of the unmasked reads.  Goes with -Z, -z and every option -O goes with; refused without -O.
 * Added: -d flags the duplicates on the GPU in front of the tally, in the same pass: every file is what this command writes without -d
 * for the input in which the duplicates carry FLAG 0x400.  A duplicate is an unpaired read that passes the filters which do not look at
 * its bases (-R, -q, -l, -L, -T, <L>M, the flags, inside its contig) and has the contig, position, length, strand and -- under -G --
 * read group of an earlier such read of the input; the first one is kept, whatever its qualities (the known difference from DeDup and
 * Picard), and the filters that look at the bases (-y, -n, -V, -Q, -U, -D) come afterwards.  Paired reads are never flagged: pairing
 * mates is out of scope.  Also writes <prefix>.pss.duplicates.txt: eligible reads, distinct keys, flagged reads, their fraction, and
 * how many keys have 1, 2, ..., 255 and more reads (duplicates.h).  With -O the BAM is the filtered, deduplicated one.  Goes with every
 * other option except -I; SAM text is fine; one GPU (PSSBAM_NGPU unset or 1): the input order defines the duplicates.
 * Added: -c and -b <file> report the depth of coverage of the tallied reads, from the same pass: a read added to a table -- exactly the
 * reads -O writes, after every filter given and after -d -- covers POS .. POS + length - 1 of its contig, mates that overlap count
 * twice, and -Q and -K change nothing.  -c writes <prefix>.pss.coverage.txt: per reference of the input's header that the FASTA
 * holds its length, covered bases, breadth, depth sum, mean and maximum depth, a total line, and the positions at depth 0..255 and
 * above (coverage.h); it is what per-base depth over the -O file of the same run gives.  -b writes the covered intervals as a
 * bedGraph (0-based, half-open, non-zero depth only, header order), what `bedtools genomecov -bg` gives for that file; it takes its
 * name when it is complete and must not name the -B or the -O file.  Either switches the engine's array on (4 bytes per genome
 * position on the device); -b alone writes no summary.  Not with -I (the span of a clipped read needs a definition of its own); SAM
 * text is fine; one GPU (PSSBAM_NGPU unset or 1): the arrays of several engines are not summed.
 * Added: -w <size> cuts every reference of the input's header that the FASTA holds into windows of <size> positions (16..2^30; the last one
 * of a contig may be short) and writes, from the same pass and the same array as -c, <prefix>.pss.windows.txt -- per window the A/C/G/T
 * letters of the FASTA, those that are C or G, their fraction, the covered positions, the summed and the mean depth of the tallied
 * reads -- and <prefix>.pss.gcbias.txt: the full-size windows with at least half of their letters A, C, G or T by GC percentage 0..100,
 * with their mean depth and that depth relative to the mean of all of them (windows.h).  It is what `bedtools makewindows | bedtools
 * coverage` and `bedtools nuc` give over the -O file, and the curve of a GC-bias plot.  -w alone writes no coverage summary.  Both files
 * take their names when they are complete.  Goes with every option -c goes with: not with -I, SAM text is fine, one GPU.
 * Added: -a <sites> [-t <n>] counts, in the same pass, the bases the tallied reads show at listed sites, split by strand: the pileup at a
 * SNP panel.  The sites file holds one site per line, contig and 1-based position in its first two blank- or tab-separated columns
 * (further columns are ignored: a `samtools mpileup -l` positions file and an ANGSD -sites file both read; '#' lines and empty lines are
 * skipped).  A read added to a table -- exactly the reads -O writes and -c counts -- shows at every listed site between its first and
 * last n bases (-t, default 0) its SEQ base there: A, C, G, T or other (N, IUPAC codes, under -Q a base below the minimum quality).
 * Writes <prefix>.pss.alleles.txt (alleles.h): per site of a contig that both the input's header and the FASTA hold -- depth 0
 * included, header order, then position -- the reference base and fA fC fG fT fO rA rC rG rT rO.  -K changes nothing.  Not with -I
 * (the offsets of a clipped or gapped read need a CIGAR walk); SAM text is fine; one GPU (PSSBAM_NGPU unset or 1).  No random or
 * majority calling and no genotype likelihoods: the counts are what such callers start from.
 * Differences on purpose: missing -F/-B/-o are detected reliably (the reference tests
 * uninitialised pointers), an unreadable FASTA/BAM is a diagnosed exit(1) instead of a
 * crash, and PSSBAM_STATS=1 prints the per-status record tallies to stderr.
 */
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "alleles.h"
#include "base_quality.h"
#include "composition.h"
#include "contig_sets.h"
#include "coverage.h"
#include "duplicates.h"
#include "end_mask.h"
#include "fasta-genome-io.h"
#include "frontend.h"
#include "interior.h"
#include "length_bins.h"
#include "length_hist.h"
#include "mismatches.h"
#include "read_groups.h"
#include "read_score.h"
#include "regions.h"
#include "replicates.h"
#include "report.h"
#include "sam_reader.h"
#include "windows.h"

/* the options' names in the messages, each spelt once */
static const char L_G[] = "-G (tables per read group)", L_S[] = "-S (tables per length bin)", L_C[] = "-C (tables per contig set)",
                  L_H[] = "-H (fragment-length histogram)", L_X[] = "-X (tables per site context)", L_E[] = "-E (tables conditional on the other end)",
                  L_I[] = "-I (clipped and gapped reads by their anchored ends)", L_A[] = "-A (tables per contig)", L_n[] = "-n (mismatch filter)",
                  L_N[] = "-N (mismatch histogram)", L_V[] = "-V (count only transversions)", L_J[] = "-J (jackknife replicates)",
                  L_W[] = "-W (read-interior table)", L_P[] = "-P (base composition around the read ends)", L_y[] = "-y (damage-score filter)",
                  L_Y[] = "-Y (damage-score histogram)";

int main(int argc, char *argv[])
{
    const double age_main = frontend_process_age_s();
    frontend_detach_start();   /* the caller gets its prompt back when the reports are written, not when 30 GB of device buffers are gone */
    const double t_main = frontend_now_s();
    int region_len = 15, min_mq = 0, merged_only = 0, by_group = 0, gapped = 0, per_contig = 0, tv_only = 0, score_hist = 0, option;
    unsigned long min_read_len = 0, max_read_len = 250000000;
    const char *up_ctx = "ACGT", *down_ctx = "ACGT";
    char *fasta_fn = NULL, *bam_fn = NULL, *out_prefix = NULL, *read_group = NULL;
    const char *len_edges = NULL, *ctg_map = NULL, *min_bq_arg = NULL, *bed_fn = NULL, *hist_arg = NULL, *site_arg = NULL, *end_arg = NULL;
    const char *max_mm_arg = NULL, *mm_hist_arg = NULL, *rep_arg = NULL, *interior_arg = NULL, *comp_arg = NULL, *min_score_arg = NULL;
    const char *out_bam = NULL, *out_level_arg = NULL;
    const char *out_mask_arg = NULL;
    int out_deflate = 0, duplicates = 0, coverage = 0;
    const char *bedgraph = NULL, *sites_fn = NULL, *trim_arg = NULL, *window_arg = NULL;
    uint32_t window = 0;

    while ((option = getopt(argc, argv, ":F:B:o:R:r:l:L:q:U:D:mGS:C:Q:T:H:X:E:IAn:N:VJ:W:P:y:YO:z:ZK:dcb:a:t:w:")) != -1) {
        switch (option) {
        case 'F': fasta_fn = strdup(optarg); break;
        case 'B': bam_fn = strdup(optarg); break;
        case 'o': out_prefix = strdup(optarg); break;
        case 'r': region_len = atoi(optarg); break;
        case 'l': min_read_len = strtoul(optarg, NULL, 10); break;
        case 'L': max_read_len = strtoul(optarg, NULL, 10); break;
        case 'q': min_mq = atoi(optarg); break;
        case 'U': up_ctx = optarg; break;
        case 'D': down_ctx = optarg; break;
        case 'm': merged_only = 1; break;
        case 'G': by_group = 1; break;
        case 'S': len_edges = optarg; break;
        case 'C': ctg_map = optarg; break;
        case 'Q': min_bq_arg = optarg; break;
        case 'T': bed_fn = optarg; break;
        case 'H': hist_arg = optarg; break;
        case 'X': site_arg = optarg; break;
        case 'E': end_arg = optarg; break;
        case 'I': gapped = 1; break;
        case 'A': per_contig = 1; break;
        case 'n': max_mm_arg = optarg; break;
        case 'N': mm_hist_arg = optarg; break;
        case 'V': tv_only = 1; break;
        case 'J': rep_arg = optarg; break;
        case 'W': interior_arg = optarg; break;
        case 'P': comp_arg = optarg; break;
        case 'y': min_score_arg = optarg; break;
        case 'Y': score_hist = 1; break;
        case 'O': out_bam = optarg; break;
        case 'z': out_level_arg = optarg; break;
        case 'Z': out_deflate = 1; break;
        case 'K': out_mask_arg = optarg; break;
        case 'd': duplicates = 1; break;
        case 'c': coverage = 1; break;
        case 'b': bedgraph = optarg; break;
        case 'a': sites_fn = optarg; break;
        case 't': trim_arg = optarg; break;
        case 'w': window_arg = optarg; break;
        case 'R': read_group = strdup(optarg); break;
        case ':':
            fprintf(stderr, "Please enter required argument for option -%c.\n", optopt);
            exit(0);
        case '?':
            if (isprint(optopt)) fprintf(stderr, "Unknown option -%c.\n", optopt);
            else fprintf(stderr, "Unknown option character \\x%x.\n", optopt);
            break;
        default:
            fprintf(stderr, "Error parsing command-line options.\n");
            exit(0);
        }
    }
    for (int i = optind; i < argc; i++) fprintf(stderr, "Non-option argument %s\n", argv[i]);

    if (!fasta_fn || !bam_fn || !out_prefix) {
        fputs("pss-bam v1.2.1: Program for describing base context and counting\n"
              "the number of matches/mismatches in aligned reads to a genome.\n"
              "-F <reference FASTA (required)>\n"
              "-B <input BAM (required)>\n"
              "-o <output filename prefix (required)>\n"
              "-r <length in basepairs into the interior of alignments to report on (default: 15)>\n"
              "-l <minimum length of read to report (default: 0)>\n"
              "-L <maximum length of read to report (default: 250000000)>\n"
              "-q <map quality filter of read to report (default: 0)>\n"
              "-R <read group name to restrict analysis to (default: all reads)>\n"
              "-U <upstream context base filter; first base before alignment must be one of these (default: ACGT)>\n"
              "-D <downstream context base filter; first base before alignment must be one of these (default: ACGT)>\n"
              "-m <only consider merged reads>\n"
              "-E <ss|ds>[,<d>] <also write the tables of each end over the reads damaged within d bases (default: 1) of the other end>\n"
              "-I <also tally clipped and gapped reads, by the matched runs at their two ends>\n"
              "-A <also write the tables of every contig of the input, one pass for any number of contigs>\n"
              "-n <k> <only tally the reads with at most k mismatches against the reference (0..255)>\n"
              "-N <M> <also write how many tallied reads have 0, 1, ..., M and more than M mismatches (1..255)>\n"
              "-V <with -n / -N: count only transversions>\n"
              "-J <K> <also write the jackknife standard errors of the rates, from K read-name replicates (2..64)>\n"
              "-W <d> <also write the substitution counts and rates of the read interior, d bases and more from both ends (0..65535)>\n"
              "-P <w> <also write the reference base composition w bases on either side of the read ends (1..30)>\n"
              "-y <t> <only tally the reads with a post-mortem-damage score of at least t nats (double-stranded model, held in units of 1/256 nat)>\n"
              "-Y <also write how many tallied reads have a post-mortem-damage score of -31 .. 30 nats and beyond; no parity with another implementation is claimed>\n"
              "-O <out.bam> <also write the tallied reads, as they are in the input and in its order, to this BAM (BAM input, one GPU)>\n"
              "-z <level> <with -O: BGZF compression level 0..9 (default: 1)>\n"
              "-Z <with -O: deflate the BAM's blocks on the GPU, not with zlib on the host (blocks cut every 0xFF00 bytes; not with -z)>\n"
              "-K <all|ds|ss>,<n5>[,<n3>] <with -O: in that BAM, mask the first n5 bases of the 5' and n3 (default: n5) of the 3' end of each read with N, quality 0: all of them, T at 5' / A at 3' (ds) or T at both (ss)>\n"
              "-d <flag duplicates before the tally: unpaired reads with the contig, position, length, strand (and, where the tables are split by read group, read group) of an earlier read; also write the duplication histogram (one GPU; not with -I)>\n"
              "-c <also write the depth of coverage of the tallied reads: per contig covered bases, breadth, mean and maximum depth, and the depth histogram (one GPU; not with -I)>\n"
              "-b <out.bedgraph> <also write the intervals the tallied reads cover, with their depth, as a bedGraph (one GPU; not with -I)>\n"
              "-w <size> <also write, per window of <size> positions (16..1073741824), the GC content of the reference and the covered positions and depth of the tallied reads, and the GC-bias table of those windows (one GPU; not with -I)>\n"
              "-a <sites.txt> <also write the bases the tallied reads show at the listed sites (contig and 1-based position per line), split by strand (one GPU; not with -I)>\n"
              "-t <n> <with -a: leave the first and last n bases of each read out of the counts (0..65535, default: 0)>\n",
              stderr);
        exit(1);
    }
    if (region_len < 0) {
        fprintf(stderr, "-r must not be negative.\n");
        exit(1);
    }
    if (by_group && read_group) {
        fprintf(stderr, "%s and -R (one read group) exclude each other.\n", L_G);
        exit(1);
    }
    if (site_arg && strcmp(site_arg, "cpg") != 0) {
        fprintf(stderr, "%s: unknown context \"%s\"; the one context is cpg.\n", L_X, site_arg);
        exit(1);
    }
    int end_depth = 0, end_cell5 = 0, end_cell3 = 0;
    if (end_arg) {   /* (the one value that is parsed before the exclusive options are checked) */
        char err[200];
        if (pss_parse_end_condition(end_arg, &end_depth, &end_cell5, &end_cell3, err, sizeof err)) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
    }
    if (tv_only && !max_mm_arg && !mm_hist_arg && !rep_arg) {
        fprintf(stderr, "%s needs %s or %s.\n", L_V, L_n, L_N);
        exit(1);
    }
    /* -O / -z: no row of the table below (the output uses no counter words; it goes with every option) */
    int out_level = 1;
    if (out_level_arg) {
        char *end = NULL;
        const long v = strtol(out_level_arg, &end, 10);
        if (!*out_level_arg || *end || v < 0 || v > 9) {
            fprintf(stderr, "-z: the compression level must be 0..9, not \"%s\".\n", out_level_arg);
            exit(1);
        }
        out_level = (int)v;
        if (!out_bam) {
            fprintf(stderr, "-z (compression level) needs -O (the BAM of the tallied reads).\n");
            exit(1);
        }
    }
    if (out_deflate && !out_bam) {
        fprintf(stderr, "-Z (deflate on the GPU) needs -O (the BAM of the tallied reads).\n");
        exit(1);
    }
    if (out_deflate && out_level_arg) {
        fprintf(stderr, "-Z deflates on the GPU, where -z (zlib's compression level) has no meaning: one or the other.\n");
        exit(1);
    }
    int out_mask_mode = PSSBAM_END_MASK_OFF;
    uint32_t out_mask_n5 = 0, out_mask_n3 = 0;
    if (out_mask_arg) {
        char err[200];
        if (pss_parse_end_mask(out_mask_arg, &out_mask_mode, &out_mask_n5, &out_mask_n3, err, sizeof err)) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
        if (!out_bam) {
            fprintf(stderr, "-K (mask the read ends) needs -O (the BAM of the tallied reads).\n");
            exit(1);
        }
    }
    if (out_bam) {
        struct stat sa, sb;
        if (!strcmp(out_bam, bam_fn) || (stat(out_bam, &sa) == 0 && stat(bam_fn, &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino)) {
            fprintf(stderr, "-O must not name the input (-B %s).\n", bam_fn);
            exit(1);
        }
        if (getenv("PSSBAM_NGPU") && atoi(getenv("PSSBAM_NGPU")) > 1) {
            fprintf(stderr, "-O writes the reads in input order, which one GPU keeps: not with PSSBAM_NGPU=%s.\n", getenv("PSSBAM_NGPU"));
            exit(1);
        }
        if (file_is_bam(bam_fn) == 0) {
            fprintf(stderr, "-O copies BAM records: it needs BAM input, and %s is SAM text.\n", bam_fn);
            exit(1);
        }
        /* (a place that cannot be written is found out now, not after the genome has been loaded) */
        char *tmp = (char *)malloc(strlen(out_bam) + 5);
        if (!tmp) { fprintf(stderr, "Error: out of memory\n"); exit(1); }
        sprintf(tmp, "%s.tmp", out_bam);
        FILE *probe = fopen(tmp, "wb");
        if (!probe) {
            fprintf(stderr, "-O: cannot create %s.\n", tmp);
            exit(1);
        }
        fclose(probe);
        remove(tmp);
        free(tmp);
    }
    /* -d: no row of the table below either (a filter in front of the tally; it goes with every option but -I) */
    if (duplicates && gapped) {
        fprintf(stderr, "-d (flag duplicates) does not go with %s: the key of a clipped read is not defined.\n", L_I);
        exit(1);
    }
    if (duplicates && getenv("PSSBAM_NGPU") && atoi(getenv("PSSBAM_NGPU")) > 1) {
        fprintf(stderr, "-d keeps the first read of a group in input order, which one GPU keeps: not with PSSBAM_NGPU=%s.\n", getenv("PSSBAM_NGPU"));
        exit(1);
    }
    /* -c / -b: no row of the table below either (they use no counter words; they go with every option but -I) */
    if ((coverage || bedgraph) && gapped) {
        fprintf(stderr, "%s does not go with %s: the span of a clipped or gapped read is not defined.\n", coverage ? "-c (depth of coverage)" : "-b (coverage bedGraph)", L_I);
        exit(1);
    }
    if ((coverage || bedgraph) && getenv("PSSBAM_NGPU") && atoi(getenv("PSSBAM_NGPU")) > 1) {
        fprintf(stderr, "%s keeps one depth array, on one GPU: not with PSSBAM_NGPU=%s.\n", coverage ? "-c" : "-b", getenv("PSSBAM_NGPU"));
        exit(1);
    }
    /* -w: the same array as -c / -b, and their rules */
    if (window_arg && pss_parse_window(window_arg, &window)) {
        fprintf(stderr, "-w takes a window size, a whole number in %u..%u, not %s.\n", PSS_WINDOW_MIN, PSS_WINDOW_MAX, window_arg);
        exit(1);
    }
    if (window_arg && gapped) {
        fprintf(stderr, "-w (windowed depth and GC content) does not go with %s: the span of a clipped or gapped read is not defined.\n", L_I);
        exit(1);
    }
    if (window_arg && getenv("PSSBAM_NGPU") && atoi(getenv("PSSBAM_NGPU")) > 1) {
        fprintf(stderr, "-w keeps one depth array, on one GPU: not with PSSBAM_NGPU=%s.\n", getenv("PSSBAM_NGPU"));
        exit(1);
    }
    /* -a / -t: no row of the table below either (no counter words; they go with every option but -I) */
    uint32_t site_trim = 0;
    if (trim_arg) {
        char *end = NULL;
        const long v = strtol(trim_arg, &end, 10);
        if (!sites_fn) {
            fprintf(stderr, "-t trims the reads of the allele counts: it needs -a <sites>.\n");
            exit(1);
        }
        if (!*trim_arg || *end || v < 0 || v > PSS_SITE_MAX_TRIM) {
            fprintf(stderr, "-t takes a number of bases in 0..%d, not %s.\n", PSS_SITE_MAX_TRIM, trim_arg);
            exit(1);
        }
        site_trim = (uint32_t)v;
    }
    if (sites_fn && gapped) {
        fprintf(stderr, "-a (allele counts at sites) does not go with %s: the offsets of a clipped or gapped read need a CIGAR walk.\n", L_I);
        exit(1);
    }
    if (sites_fn && getenv("PSSBAM_NGPU") && atoi(getenv("PSSBAM_NGPU")) > 1) {
        fprintf(stderr, "-a keeps one set of site counters, on one GPU: not with PSSBAM_NGPU=%s.\n", getenv("PSSBAM_NGPU"));
        exit(1);
    }
    if (bedgraph) {
        const struct { const char *what, *path; } others[] = {{"the input (-B", bam_fn}, {"the BAM of the tallied reads (-O", out_bam}};
        for (size_t i = 0; i < sizeof others / sizeof *others; i++) {
            struct stat sa, sb;
            const char *path = others[i].path;
            if (path && (!strcmp(bedgraph, path) || (stat(bedgraph, &sa) == 0 && stat(path, &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino))) {
                fprintf(stderr, "-b must not name %s %s).\n", others[i].what, path);
                exit(1);
            }
        }
        /* (a place that cannot be written is found out now, not after the genome has been loaded; a file that is there already
         * under the temporary name is opened for appending and left as it is) */
        char *tmp = (char *)malloc(strlen(bedgraph) + 5);
        if (!tmp) { fprintf(stderr, "Error: out of memory\n"); exit(1); }
        sprintf(tmp, "%s.tmp", bedgraph);
        const int was_there = access(tmp, F_OK) == 0;
        FILE *probe = fopen(tmp, "a");
        if (!probe) {
            fprintf(stderr, "-b: cannot create %s.\n", tmp);
            exit(1);
        }
        fclose(probe);
        if (!was_there) remove(tmp);
        free(tmp);
    }
    /* The exclusive options: at most one row may be given (their tables share the words behind the engine's planes, and
     * one pass over 32 table rows).  Of two, the later row is named first, by all it was given with, the earlier one by
     * its first option.  A new option is one row here. */
    const char *mism_one = max_mm_arg ? L_n : mm_hist_arg ? L_N : L_V, *score_one = min_score_arg ? L_y : L_Y;
    const char *mism_all = max_mm_arg && mm_hist_arg ? "-n / -N (mismatch filter and histogram)" : mism_one;
    const char *score_all = min_score_arg && score_hist ? "-y / -Y (damage-score filter and histogram)" : score_one;
    const struct { int given; const char *mine, *other; } exclusive[] = {
        {by_group, L_G, L_G},
        {len_edges != NULL, L_S, L_S},
        {ctg_map != NULL, L_C, L_C},
        {hist_arg != NULL, L_H, L_H},
        {site_arg != NULL, L_X, L_X},
        {end_arg != NULL, L_E, L_E},
        {gapped, L_I, L_I},
        {per_contig, L_A, L_A},
        {max_mm_arg || mm_hist_arg || tv_only, mism_all, mism_one},
        {rep_arg != NULL, L_J, L_J},
        {interior_arg != NULL, L_W, L_W},
        {comp_arg != NULL, L_P, L_P},
        {min_score_arg || score_hist, score_all, score_one},
    };
    const char *other = NULL;
    for (size_t i = 0; i < sizeof exclusive / sizeof *exclusive; i++) {
        if (!exclusive[i].given) continue;
        if (other) {
            fprintf(stderr, "%s and %s exclude each other.\n", exclusive[i].mine, other);
            exit(1);
        }
        other = exclusive[i].other;
    }
    uint32_t edges[PSSBAM_MAX_LENGTH_BINS - 1];
    int n_edges = 0;
    if (len_edges) {
        char err[200];
        if ((n_edges = pss_parse_length_edges(len_edges, min_read_len, max_read_len, edges, err, sizeof err)) < 0) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
    }
    int min_bq = 0;
    if (min_bq_arg) {
        char err[200];
        if ((min_bq = pss_parse_min_base_quality(min_bq_arg, err, sizeof err)) < 0) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
    }
    int hist_max = 0;
    if (hist_arg) {
        char err[200];
        if ((hist_max = pss_parse_length_hist(hist_arg, err, sizeof err)) < 0) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
    }
    if (end_arg && (region_len > 30 || end_depth > region_len)) {
        fprintf(stderr, "%s needs its depth <= -r <= 30 (both ends' marks are taken from the one pass "
                        "over 32 table rows), not -r %d with depth %d.\n", L_E, region_len, end_depth);
        exit(1);
    }
    int replicates = 0;
    if (rep_arg) {
        char err[200];
        if ((replicates = pss_parse_replicates(rep_arg, err, sizeof err)) < 0) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
    }
    int max_mm = -1, mm_hist = 0;
    if (max_mm_arg || mm_hist_arg) {
        char err[200];
        if ((max_mm_arg && (max_mm = pss_parse_max_mismatches(max_mm_arg, err, sizeof err)) < 0) ||
            (mm_hist_arg && (mm_hist = pss_parse_mismatch_hist(mm_hist_arg, err, sizeof err)) < 0)) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
        if (region_len > 30) {
            fprintf(stderr, "%s needs -r <= 30 (a read's fate is decided in the one pass over 32 table rows), not -r %d.\n", mism_all, region_len);
            exit(1);
        }
    }
    int interior = -1;
    if (interior_arg) {
        char err[200];
        if ((interior = pss_parse_interior_margin(interior_arg, err, sizeof err)) < 0) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
        if (region_len > 30) {
            fprintf(stderr, "%s needs -r <= 30 (a read's fate is decided in the one pass over 32 table rows), not -r %d.\n", L_W, region_len);
            exit(1);
        }
    }
    int composition = 0;
    if (comp_arg) {
        char err[200];
        if ((composition = pss_parse_composition_width(comp_arg, err, sizeof err)) < 0) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
        if (region_len > 30) {
            fprintf(stderr, "%s needs -r <= 30 (a read's fate and its end windows are those of the one pass over 32 table rows), not -r %d.\n", L_P, region_len);
            exit(1);
        }
    }
    static int16_t pmd_weights[4 * PSS_PMD_DIST * PSS_PMD_QUAL];
    static frontend_score score;
    if (min_score_arg || score_hist) {
        int32_t min_score = 0;
        char err[200];
        if (min_score_arg && pss_parse_min_score(min_score_arg, &min_score, err, sizeof err)) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
        if (region_len > 30) {
            fprintf(stderr, "%s needs -r <= 30 (a read's fate is decided in the one pass over 32 table rows), not -r %d.\n", score_all, region_len);
            exit(1);
        }
        pss_pmd_weights(pmd_weights);
        score.weights = pmd_weights;
        score.n_dist = PSS_PMD_DIST;
        score.n_qual = PSS_PMD_QUAL;
        score.use_filter = min_score_arg != NULL;
        score.min_score = min_score;
        score.hist_half = score_hist ? PSS_PMD_HIST_HALF : 0;
        score.hist_shift = score_hist ? PSS_PMD_HIST_SHIFT : 0;
    }
    pss_regions bed;
    memset(&bed, 0, sizeof bed);
    if (bed_fn) {
        char err[300];
        if (pss_read_bed(bed_fn, &bed, err, sizeof err)) {
            fprintf(stderr, "%s (%s)\n", err, bed_fn);
            exit(1);
        }
    }
    pss_sites sites;
    memset(&sites, 0, sizeof sites);
    if (sites_fn) {
        char err[600];
        if (pss_read_sites(sites_fn, &sites, err, sizeof err)) {
            fprintf(stderr, "%s\n", err);
            exit(1);
        }
    }
    frontend_contig_map sets;
    memset(&sets, 0, sizeof sets);
    if (ctg_map) {
        FILE *mf = fopen(ctg_map, "rb");
        char *text = NULL;
        size_t len = 0, cap = 0;
        int read_ok = mf != NULL;
        while (read_ok) {
            if (len == cap) {
                char *t = (char *)realloc(text, cap = cap ? 2 * cap : 65536);
                if (!t) { read_ok = 0; break; }
                text = t;
            }
            const size_t got = fread(text + len, 1, cap - len, mf);
            len += got;
            if (got == 0) { read_ok = !ferror(mf); break; }
        }
        if (mf) fclose(mf);
        if (!read_ok) {
            fprintf(stderr, "-C: unable to read the map file %s.\n", ctg_map);
            exit(1);
        }
        char err[600];
        sets.n_names = pss_parse_contig_sets(text, len, &sets.names, &sets.set_of, &sets.labels, &sets.n_labels, err, sizeof err);
        free(text);
        if (sets.n_names < 0) {
            fprintf(stderr, "%s (%s)\n", err, ctg_map);
            exit(1);
        }
    }

    /* "Full command" banner: four shapes, as the reference prints them (pss-bam.c:728-749) */
    fprintf(stderr, "Full command: %s -F %s -B %s -o %s -r %d -l %lu -L %lu -q %d", argv[0], fasta_fn, bam_fn,
            out_prefix, region_len, min_read_len, max_read_len, min_mq);
    if (read_group) fprintf(stderr, " -R %s", read_group);
    fprintf(stderr, " -U %s -D %s%s%s", up_ctx, down_ctx, merged_only ? " -m" : "", by_group ? " -G" : "");
    if (len_edges) fprintf(stderr, " -S %s", len_edges);
    if (ctg_map) fprintf(stderr, " -C %s", ctg_map);
    if (min_bq_arg) fprintf(stderr, " -Q %d", min_bq);
    if (hist_arg) fprintf(stderr, " -H %d", hist_max);
    if (site_arg) fprintf(stderr, " -X %s", site_arg);
    if (end_arg) fprintf(stderr, " -E %s", end_arg);
    if (gapped) fprintf(stderr, " -I");
    if (per_contig) fprintf(stderr, " -A");
    if (max_mm_arg) fprintf(stderr, " -n %d", max_mm);
    if (mm_hist_arg) fprintf(stderr, " -N %d", mm_hist);
    if (tv_only) fprintf(stderr, " -V");
    if (rep_arg) fprintf(stderr, " -J %d", replicates);
    if (interior_arg) fprintf(stderr, " -W %d", interior);
    if (comp_arg) fprintf(stderr, " -P %d", composition);
    if (min_score_arg) fprintf(stderr, " -y %s", min_score_arg);
    if (score_hist) fprintf(stderr, " -Y");
    if (out_bam && out_deflate) fprintf(stderr, " -O %s -Z", out_bam);
    else if (out_bam) fprintf(stderr, " -O %s -z %d", out_bam, out_level);
    if (out_mask_arg) fprintf(stderr, " -K %s,%u,%u", out_mask_mode == PSSBAM_END_MASK_ALL ? "all" : out_mask_mode == PSSBAM_END_MASK_DS ? "ds" : "ss", out_mask_n5, out_mask_n3);
    if (duplicates) fprintf(stderr, " -d");
    if (coverage) fprintf(stderr, " -c");
    if (bedgraph) fprintf(stderr, " -b %s", bedgraph);
    if (window_arg) fprintf(stderr, " -w %u", window);
    if (sites_fn) fprintf(stderr, " -a %s -t %u", sites_fn, site_trim);
    fputc('\n', stderr);

    pssbam_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = PSSBAM_ABI_VERSION;
    cfg.tally_mask = PSSBAM_TALLY_PSS;
    cfg.pss.region_len = region_len;
    cfg.pss.min_read_len = min_read_len;
    cfg.pss.max_read_len = max_read_len;
    cfg.pss.min_mq = min_mq;
    cfg.pss.up_ctx = up_ctx;
    cfg.pss.down_ctx = down_ctx;
    cfg.pss.merged_only = merged_only;
    cfg.read_group = read_group;
    cfg.device = 0;
    cfg.kernel = PSSBAM_KERNEL_AUTO;

    frontend_opts.group_by_rg = by_group;
    frontend_opts.n_length_edges = n_edges;
    memcpy(frontend_opts.length_edges, edges, (size_t)n_edges * sizeof *edges);
    if (ctg_map) frontend_opts.contig_sets = &sets;
    frontend_opts.min_base_quality = min_bq;
    frontend_opts.length_hist = hist_max;
    frontend_opts.site_context = site_arg ? PSSBAM_SITE_CPG : PSSBAM_SITE_NONE;
    frontend_opts.end_depth = end_depth;
    frontend_opts.end_cell5 = end_cell5;
    frontend_opts.end_cell3 = end_cell3;
    frontend_opts.gapped_reads = gapped;
    frontend_opts.per_contig = per_contig;
    frontend_opts.mismatch_hist = mm_hist;
    frontend_opts.max_mismatches = max_mm;
    frontend_opts.mismatch_tv = tv_only;
    frontend_opts.replicates = replicates;
    frontend_opts.interior = interior;
    frontend_opts.composition = composition;
    if (score.weights) frontend_opts.read_score = &score;
    if (bed_fn) frontend_opts.regions = &bed;
    frontend_opts.out_bam = out_bam;
    frontend_opts.out_level = out_level;
    frontend_opts.out_deflate = out_deflate;
    frontend_opts.out_mask_mode = out_mask_mode;
    frontend_opts.out_mask_n5 = out_mask_n5;
    frontend_opts.out_mask_n3 = out_mask_n3;
    frontend_opts.duplicates = duplicates;
    frontend_opts.coverage = coverage;
    frontend_opts.coverage_bedgraph = bedgraph;
    frontend_opts.coverage_window = window;
    frontend_opts.sites = sites_fn ? &sites : NULL;
    frontend_opts.site_trim = site_trim;
    fprintf(stderr, "Reading genome sequence from:\n%s\n", fasta_fn);
    /* HIP start-up, engines and the compressed BAM feed (PCIe, inflate, CRC, record index) overlap the FASTA
     * load; only the tally launches wait for the genome (frontend.c) */
    frontend_warmup_start(&cfg, bam_fn, fasta_fn);
    const double t_fa = frontend_now_s();
    Genome *genome = init_genome(fasta_fn);
    if (getenv("PSSBAM_STATS")) fprintf(stderr, "[pssbam] genome: fasta load %.3f s\n", frontend_now_s() - t_fa);
    if (!genome) {
        fprintf(stderr, "Error: Unable to load genome from %s.\n", fasta_fn);
        front_end_fail(1);   /* (not exit(): the helper thread may still be starting the HIP runtime up) */
    }
    fprintf(stderr, "Finished loading genome.\nCounting matches/mismatches from:\n%s\n", bam_fn);

    run_result res;
    frontend_fast_exit = getenv("PSSBAM_CLEAN_EXIT") == NULL;
    if (run_tally(&cfg, genome, bam_fn, env_gpu_count(), &res)) exit(1);

    double *fwd_rates = (double *)calloc((size_t)(region_len ? region_len : 1) * 12, sizeof(double));
    double *rev_rates = (double *)calloc((size_t)(region_len ? region_len : 1) * 12, sizeof(double));
    pss_sub_rates(region_len, res.fwd, fwd_rates);
    pss_sub_rates(region_len, res.rev, rev_rates);
    pss_write_counts(fasta_fn, bam_fn, out_prefix, region_len, res.fwd, res.rev);
    pss_write_rates(fasta_fn, bam_fn, out_prefix, region_len, fwd_rates, rev_rates);
    if (res.hist_fwd && pss_write_lengths(fasta_fn, bam_fn, out_prefix, res.hist_max, res.hist_fwd, res.hist_rev)) exit(1);
    if (res.mism_fwd && pss_write_mismatches(fasta_fn, bam_fn, out_prefix, res.mism_max, tv_only, res.mism_fwd, res.mism_rev)) exit(1);   /* -N */
    if (res.has_interior && pss_write_interior(fasta_fn, bam_fn, out_prefix, interior, min_bq, res.interior, res.interior_reads)) exit(1);   /* -W */
    if (res.comp5 && pss_write_composition(fasta_fn, bam_fn, out_prefix, res.composition_width, res.comp5, res.comp3)) exit(1);   /* -P */
    if (res.score_fwd && pss_write_read_scores(fasta_fn, bam_fn, out_prefix, res.score_half, res.score_fwd, res.score_rev)) exit(1);   /* -Y */
    if (res.has_duplicates && pss_write_duplicates(fasta_fn, bam_fn, out_prefix, "pss", res.dup_totals, res.dup_hist, PSS_DUP_HIST_MAX)) exit(1);   /* -d */
    if (res.has_coverage && coverage &&
        pss_write_coverage(fasta_fn, bam_fn, out_prefix, res.cov_n, (const char *const *)res.cov_names, res.cov_held, res.cov_lengths, res.cov_per_contig, res.cov_hist,
                           PSS_COV_HIST_MAX))
        exit(1);   /* -c */
    if (res.has_coverage && bedgraph &&
        pss_write_coverage_bedgraph(bedgraph, res.cov_n, (const char *const *)res.cov_names, res.cov_n_runs, res.cov_run_ref, res.cov_run_start, res.cov_run_end,
                                    res.cov_run_depth))
        exit(1);   /* -b */
    if (res.has_coverage && window &&
        pss_write_windows(fasta_fn, bam_fn, out_prefix, window, res.cov_n, (const char *const *)res.cov_names, res.win_n, res.win_ref, res.win_start, res.win_end,
                          res.win_acgt, res.win_gc, res.win_covered, res.win_depth_sum))
        exit(1);   /* -w */
    if (res.has_alleles &&
        pss_write_alleles(fasta_fn, bam_fn, sites_fn, site_trim, out_prefix, res.allele_n_names, (const char *const *)res.allele_names, res.allele_n, res.allele_ref,
                          res.allele_pos, res.allele_base, res.allele_counts, res.allele_totals))
        exit(1);   /* -a */
    if (res.site_fwd) {   /* -X: IN as the engine returns it; OUT = T - IN on the position rows, the context rows as T */
        const size_t cells = (size_t)(region_len + 2) * 16;
        unsigned long *out_fwd = (unsigned long *)malloc(cells * sizeof *out_fwd), *out_rev = (unsigned long *)malloc(cells * sizeof *out_rev);
        if (!out_fwd || !out_rev) { fprintf(stderr, "Error: out of memory\n"); exit(1); }
        for (size_t i = 0; i < cells; i++) {
            out_fwd[i] = i < 32 ? res.fwd[i] : res.fwd[i] - res.site_fwd[i];
            out_rev[i] = i < 32 ? res.rev[i] : res.rev[i] - res.site_rev[i];
        }
        if (pss_write_labelled(fasta_fn, bam_fn, out_prefix, "cpg", region_len, res.site_fwd, res.site_rev) ||
            pss_write_labelled(fasta_fn, bam_fn, out_prefix, "noncpg", region_len, out_fwd, out_rev)) exit(1);
        free(out_fwd);
        free(out_rev);
    }
    if (res.end_fwd && (pss_write_labelled(fasta_fn, bam_fn, out_prefix, "cond", region_len, res.end_fwd, res.end_rev) ||
                        pss_write_end_reads(out_prefix, res.end_reads))) exit(1);   /* -E */
    if (per_contig && pss_write_contigs(fasta_fn, bam_fn, out_prefix, region_len, res.n_contigs, (const char *const *)res.contig_names,
                                        res.contig_fwd, res.contig_rev)) exit(1);   /* -A */
    if (replicates) {   /* -J: the planes are the replicates' tables; no file per replicate */
        const size_t n_rates = (size_t)(region_len ? region_len : 1) * 12;
        double *fwd_se = (double *)calloc(n_rates, sizeof(double)), *rev_se = (double *)calloc(n_rates, sizeof(double));
        if (!fwd_se || !rev_se || res.n_planes != replicates || pss_jackknife_se(region_len, replicates, res.fwd, res.plane_fwd, fwd_se) ||
            pss_jackknife_se(region_len, replicates, res.rev, res.plane_rev, rev_se)) {
            fprintf(stderr, "Error: out of memory\n");
            exit(1);
        }
        if (pss_write_rates_se(fasta_fn, bam_fn, out_prefix, region_len, replicates, fwd_se, rev_se)) exit(1);
        free(fwd_se);
        free(rev_se);
    }
    if (by_group && res.n_planes == 0)
        fprintf(stderr, "Warning: -G: the header of %s has no @RG line; only the tables of all reads were written.\n", bam_fn);
    /* <prefix>.<tag>: what `-R <ID> -o <prefix>.<ID>` (-G), `-l <lo> -L <hi> -o <prefix>.len<lo>-<hi>` (-S) or -F
     * reduced to the label's contigs with `-o <prefix>.<label>` (-C) writes */
    for (int k = 0; k < res.n_planes && !replicates; k++) {
        const size_t cells = (size_t)(region_len + 2) * 16;
        unsigned long lo = 0, hi = 0;
        if (len_edges) pss_length_bin_bounds(edges, n_edges, k, min_read_len, max_read_len, &lo, &hi);
        const char *id = by_group ? res.group_ids[k] : ctg_map ? sets.labels[k] : NULL;   /* file-name encoded */
        const size_t tag_len = id ? pss_rg_file_tag(id, NULL, 0) : pss_length_bin_tag(lo, hi, NULL, 0);
        char *pprefix = (char *)malloc(strlen(out_prefix) + tag_len + 2);
        if (!pprefix) { fprintf(stderr, "Error: out of memory\n"); exit(1); }
        char *tag = pprefix + sprintf(pprefix, "%s.", out_prefix);
        if (id) pss_rg_file_tag(id, tag, tag_len + 1);
        else pss_length_bin_tag(lo, hi, tag, tag_len + 1);
        pss_sub_rates(region_len, res.plane_fwd + k * cells, fwd_rates);
        pss_sub_rates(region_len, res.plane_rev + k * cells, rev_rates);
        pss_write_counts(fasta_fn, bam_fn, pprefix, region_len, res.plane_fwd + k * cells, res.plane_rev + k * cells);
        pss_write_rates(fasta_fn, bam_fn, pprefix, region_len, fwd_rates, rev_rates);
        free(pprefix);
    }

    if (getenv("PSSBAM_STATS")) {
        static const char *nm[] = {"records", "rg_dropped", "parse_skip", "no_contig", "pss_ok", "pss_filtered"};
        for (int i = 0; i < 6; i++) fprintf(stderr, "[pssbam] %s=%llu\n", nm[i], (unsigned long long)res.stats[i]);
        fprintf(stderr, "[pssbam] slow_path=%llu%s\n", (unsigned long long)res.stats[PSSBAM_ST_SLOW_PATH],
                res.stats[PSSBAM_ST_SLOW_PATH] * 100 > res.stats[PSSBAM_ST_RECORDS]
                    ? "  (more than 1 % of the records were longer than the staged prefix and took the one-lane path: slower, same tables)" : "");
        fprintf(stderr, "[pssbam] gpus=%d inflate_s=%.3f total_s=%.3f\n", res.n_gpus, res.inflate_s, res.total_s);
        fprintf(stderr, "[pssbam] main() to reports written: %.3f s\n", frontend_now_s() - t_main);
        fprintf(stderr, "[pssbam] process creation to main(): %.2f s (exec + dynamic loading); main() to here %.3f s; exit: %s\n", age_main,
                frontend_now_s() - t_main, frontend_detached() ? "the caller is released now, this worker is torn down behind it" : "one process, teardown in the foreground");
    }
    if (frontend_fast_exit) { /* nothing left to do but to hand the memory back: let the OS */
        fprintf(stderr, "Done.\n");
        front_end_exit(0);
    }
    free(fwd_rates);
    free(rev_rates);
    run_result_free(&res);
    if (ctg_map) pss_free_contig_sets(sets.names, sets.n_names, sets.set_of, sets.labels, sets.n_labels);
    destroy_genome(genome);
    free(fasta_fn);
    free(bam_fn);
    free(out_prefix);
    free(read_group);
    fprintf(stderr, "Done.\n");
    return 0;
}

/*
 * pss-bam_amd/host/fragkon_main.c -- the `fragkon` command, MI355X edition.
 *
 * Same options, stderr banners and stdout table as the reference front end
 * (/root/reference/fragkon.c:253-386); the k-mer tallies come from the GPU engine's flat
 * 4^k histograms (k <= 15 on the device).  See pss_main.c for what differs underneath.
 * Added, as in pss-bam: -G, -S e1,...,ek and -C <map file> (at most one of them, with -o <prefix>) write, beside the
 * table of all reads on stdout, one table per @RG ID, per read-length bin or per label of the map to
 * <prefix>.<tag>.fragkon.txt (the tags pss-bam uses), each what the same command prints for that plane alone:
 * on the records `samtools view -r <ID>` keeps, with `-l <lo> -L <hi>`, or with -F cut down to the label's
 * contigs -- from one pass over the input.  Without these options nothing differs from the reference front end.
 * Added: -T <bed> tallies only the reads whose alignment overlaps an interval of the BED file, as in pss-bam: every
 * table is what this command gives without -T for the input reduced by `samtools view -L <bed>`.
 * Added: -d flags the duplicates on the GPU in front of the tally, as in pss-bam (pss_main.c has the definition; eligible here =
 * an unpaired candidate of this command's own filters): every table is what this command gives without -d for the input whose
 * duplicates carry FLAG 0x400.  With -o it also writes <prefix>.fragkon.duplicates.txt (duplicates.h).  One GPU.
 * pss-bam's -c / -b (depth of coverage of the tallied reads) are refused: the candidates of the k-mer tables are not the reads of a table.
 * So is its -w (windowed depth and GC content), which reads the same array.
 * So are its -a / -t (allele counts of the tallied reads at listed sites), for the same reason.
 */
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "contig_sets.h"
#include "fasta-genome-io.h"
#include "frontend.h"
#include "length_bins.h"
#include "read_groups.h"
#include "regions.h"
#include "report.h"
#include "sam-parse.h"

int main(int argc, char *argv[])
{
    frontend_detach_start();   /* (frontend.c: the caller does not wait for the teardown) */
    int klen = 8, min_mq = 0, merged_only = 0, option;
    unsigned long min_read_len = 0, max_read_len = 250000000;
    char *fasta_fn = NULL, *bam_fn = NULL, *out_prefix = NULL;
    int by_group = 0, duplicates = 0;
    const char *len_edges = NULL, *ctg_map = NULL, *bed_fn = NULL;

    while ((option = getopt(argc, argv, ":F:B:k:l:L:q:mGS:C:o:T:dcb:a:t:w:")) != -1) {
        switch (option) {
        case 'F': fasta_fn = strdup(optarg); break;
        case 'B': bam_fn = strdup(optarg); break;
        case 'k': klen = atoi(optarg); break;
        case 'l': min_read_len = strtoul(optarg, NULL, 10); break;
        case 'L': max_read_len = strtoul(optarg, NULL, 10); break;
        case 'q': min_mq = atoi(optarg); break;
        case 'm': merged_only = 1; break;
        case 'G': by_group = 1; break;
        case 'S': len_edges = optarg; break;
        case 'C': ctg_map = optarg; break;
        case 'T': bed_fn = optarg; break;
        case 'd': duplicates = 1; break;
        case 'c':
        case 'b':   /* pss-bam's depth of coverage is that of the reads in its tables; this command's candidates are not those */
            fprintf(stderr, "-%c (depth of coverage of the tallied reads) is an option of pss-bam: fragkon has none.\n", option);
            exit(1);
        case 'w':   /* ... and so is the depth of its windows */
            fprintf(stderr, "-%c (windowed depth and GC content of the tallied reads) is an option of pss-bam: fragkon has none.\n", option);
            exit(1);
        case 'a':
        case 't':   /* likewise pss-bam's allele counts at listed sites */
            fprintf(stderr, "-%c (allele counts of the tallied reads at listed sites) is an option of pss-bam: fragkon has none.\n", option);
            exit(1);
        case 'o': out_prefix = strdup(optarg); break;
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

    if (!fasta_fn || !bam_fn) {
        fputs("fragkon: Program for describing kmer-based genomic sequence\n"
              "contexts around the fragmentation points of aligned reads.\n"
              "-F <reference FASTA (required)>\n"
              "-B <input BAM (required)>\n"
              "-k <kmer length (default: 8)>\n"
              "-l <minimum length of read to report (default: 0)>\n"
              "-L <maximum length of read to report (default: 250000000)>\n"
              "-q <map quality filter of read to report (default: 0)>\n"
              "-m <only consider merged reads>\n"
              "-d <flag duplicates before the tally: unpaired reads with the contig, position, length, strand (and, where the tables are split by read group, read group) of an earlier read; with -o, also write the duplication histogram (one GPU)>\n",
              stderr);
        exit(1);
    }
    const int n_selectors = by_group + (len_edges != NULL) + (ctg_map != NULL);
    if (n_selectors > 1) {
        fprintf(stderr, "-G (tables per read group), -S (tables per length bin) and -C (tables per contig set) exclude each other.\n");
        exit(1);
    }
    if (n_selectors && !out_prefix) {
        fprintf(stderr, "-%c needs -o <output filename prefix> for the per-%s tables (<prefix>.<tag>.fragkon.txt).\n",
                by_group ? 'G' : len_edges ? 'S' : 'C', by_group ? "read-group" : len_edges ? "length-bin" : "contig-set");
        exit(1);
    }
    if (duplicates && getenv("PSSBAM_NGPU") && atoi(getenv("PSSBAM_NGPU")) > 1) {
        fprintf(stderr, "-d keeps the first read of a group in input order, which one GPU keeps: not with PSSBAM_NGPU=%s.\n", getenv("PSSBAM_NGPU"));
        exit(1);
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
    pss_regions bed;
    memset(&bed, 0, sizeof bed);
    if (bed_fn) {
        char err[300];
        if (pss_read_bed(bed_fn, &bed, err, sizeof err)) {
            fprintf(stderr, "%s (%s)\n", err, bed_fn);
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
    if (klen < 1 || klen > PSSBAM_MAX_KLEN) {
        fprintf(stderr, "k-mer length %d is outside the range this build tallies on the GPU (1..%d).\n", klen, PSSBAM_MAX_KLEN);
        exit(1);
    }

    fputs("# Entered command: ", stderr);
    for (int i = 0; i < argc; i++) fprintf(stderr, "%s ", argv[i]);
    fputc('\n', stderr);
    fprintf(stderr, "Input kmer length = %d.\n", klen);
    if (klen & 1)
        fprintf(stderr, "    *** k is odd - counting %d bases outside %d bases inside of alignment.\n", klen / 2,
                klen / 2 + 1);
    fprintf(stderr, "Reading genome sequence from: %s\n", fasta_fn);
    pssbam_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.abi_version = PSSBAM_ABI_VERSION;
    cfg.tally_mask = PSSBAM_TALLY_KMER;
    cfg.kmer.klen = klen;
    cfg.kmer.min_mq = min_mq;
    cfg.kmer.min_read_len = min_read_len;
    cfg.kmer.max_read_len = max_read_len;
    cfg.kmer.merged_only = merged_only;
    cfg.device = 0;
    cfg.kernel = PSSBAM_KERNEL_AUTO;

    frontend_opts.group_by_rg = by_group;
    frontend_opts.n_length_edges = n_edges;
    memcpy(frontend_opts.length_edges, edges, (size_t)n_edges * sizeof *edges);
    if (ctg_map) frontend_opts.contig_sets = &sets;
    if (bed_fn) frontend_opts.regions = &bed;
    frontend_opts.duplicates = duplicates;   /* -d: pss-bam's, for the k-mer tables (pss_main.c) */
    /* HIP start-up, engines and the compressed BAM feed overlap the FASTA load (frontend.c) */
    frontend_warmup_start(&cfg, bam_fn, fasta_fn);
    Genome *genome = init_genome(fasta_fn);
    if (!genome) {
        fprintf(stderr, "Error: Unable to load genome from %s.\n", fasta_fn);
        front_end_fail(1);   /* (not exit(): the helper thread may still be starting the HIP runtime up) */
    }
    fprintf(stderr, "Finished loading genome.\nCounting kmer contexts for: %s\n", bam_fn);

    run_result res;
    frontend_fast_exit = getenv("PSSBAM_CLEAN_EXIT") == NULL;
    if (run_tally(&cfg, genome, bam_fn, env_gpu_count(), &res)) exit(1);
    fragkon_write_table(stdout, fasta_fn, bam_fn, klen, res.k5, res.k3);
    fflush(stdout);
    /* -d: <prefix>.fragkon.duplicates.txt, only when there is a prefix to write it under */
    if (res.has_duplicates && out_prefix && pss_write_duplicates(fasta_fn, bam_fn, out_prefix, "fragkon", res.dup_totals, res.dup_hist, PSS_DUP_HIST_MAX)) exit(1);
    if (by_group && res.n_planes == 0)
        fprintf(stderr, "Warning: -G: the header of %s has no @RG line; only the table of all reads was written.\n", bam_fn);
    /* <prefix>.<tag>.fragkon.txt: what the same command prints for the plane's records alone */
    for (int k = 0; k < res.n_planes; k++) {
        const size_t bins = (size_t)1 << (2 * klen);
        unsigned long lo = 0, hi = 0;
        if (len_edges) pss_length_bin_bounds(edges, n_edges, k, min_read_len, max_read_len, &lo, &hi);
        const char *id = by_group ? res.group_ids[k] : ctg_map ? sets.labels[k] : NULL;   /* file-name encoded */
        const size_t tag_len = id ? pss_rg_file_tag(id, NULL, 0) : pss_length_bin_tag(lo, hi, NULL, 0);
        char *tag = (char *)malloc(tag_len + 1);
        if (!tag) { fprintf(stderr, "Error: out of memory\n"); exit(1); }
        if (id) pss_rg_file_tag(id, tag, tag_len + 1);
        else pss_length_bin_tag(lo, hi, tag, tag_len + 1);
        if (fragkon_write_plane(fasta_fn, bam_fn, out_prefix, tag, klen, res.plane_k5 + k * bins, res.plane_k3 + k * bins)) exit(1);
        free(tag);
    }
    if (getenv("PSSBAM_STATS")) {
        fprintf(stderr, "[pssbam] records=%llu kmer_ok=%llu kmer_filtered=%llu kmer_fail=%llu gpus=%d\n",
                (unsigned long long)res.stats[PSSBAM_ST_RECORDS], (unsigned long long)res.stats[PSSBAM_ST_KMER_OK],
                (unsigned long long)res.stats[PSSBAM_ST_KMER_FILTERED], (unsigned long long)res.stats[PSSBAM_ST_KMER_FAIL],
                res.n_gpus);
    }
    if (frontend_fast_exit) { /* nothing left to do but to hand the memory back: let the OS */
        fprintf(stderr, "Done.\n");
        front_end_exit(0);
    }
    run_result_free(&res);
    destroy_genome(genome);
    if (ctg_map) pss_free_contig_sets(sets.names, sets.n_names, sets.set_of, sets.labels, sets.n_labels);
    free(fasta_fn);
    free(bam_fn);
    free(out_prefix);
    fprintf(stderr, "Done.\n");
    return 0;
}

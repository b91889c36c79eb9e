/* pss-bam_amd/host/alleles.h -- pss-bam -a / -t: the sites-file reader and the report of the allele counts at the listed sites
 * (include/pssbam_hip.h: pssbam_engine_set_sites). */
#ifndef PSSBAM_ALLELES_H
#define PSSBAM_ALLELES_H

#include <stddef.h>
#include <stdint.h>

#define PSS_SITE_MAX_TRIM 65535

/* the sites as pssbam_engine_set_sites takes them: site i is the 0-based position pos0[i] on contig names[name_of[i]] */
typedef struct pss_sites {
    int32_t n_names;
    char **names;
    int64_t n;
    int32_t *name_of;
    uint32_t *pos0;
} pss_sites;

/* Parses a sites file held in memory: one site per line, fields separated by blanks or tabs, the first two the contig and the
 * 1-based position; further columns are ignored (a `samtools mpileup -l` positions file and an ANGSD -sites file both read).  Lines
 * that are empty or start with '#' are skipped, a CR in front of the LF is dropped.  `path` only names the file in messages.
 * Returns 0, or -1 with a message in err that names the file and the line: fewer than two fields, a position that is not a decimal
 * integer, is 0 or is above 2^32, more than PSSBAM_MAX_REGIONS sites, or no site at all. */
int pss_parse_sites(const char *path, const char *text, size_t len, pss_sites *out, char *err, size_t err_cap);
/* the same for a file; a gzip file is refused */
int pss_read_sites(const char *path, pss_sites *out, char *err, size_t err_cap);
void pss_free_sites(pss_sites *s);

/* Writes <out_prefix>.pss.alleles.txt, as <...>.tmp that takes its name when it is complete (a failure leaves neither): two '#'
 * lines (the files and the trim; totals = pssbam_engine_finish_sites': given, resolved, covered, bases), the column line, and one
 * line per resolved site in the order given -- contig names[ref[i]] (n_names of them), 1-based position, reference base, the ten
 * counters fA fC fG fT fO rA rC rG rT rO.  Returns 0, or 1 after a message on stderr. */
int pss_write_alleles(const char *fasta_fn, const char *bam_fn, const char *sites_fn, uint32_t trim, const char *out_prefix, int n_names,
                      const char *const *names, uint64_t n_sites, const int32_t *ref, const uint32_t *pos0, const uint8_t *ref_base,
                      const uint32_t *counts, const uint64_t totals[4]);

#endif

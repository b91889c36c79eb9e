/*
 * include/pssbam_hip.h -- C ABI of the MI355X (gfx950) tally engine.
 *
 * This is the drop-in boundary for pss-bam's per-read hot path.  The reference has no
 * FFI seam; the loop it replaces is
 *
 *     while (fgets(line)) { line2saml(line, sp); process_aln(fwd, rev, genome, sp); }
 *         /root/reference/pss-bam.c:764-783   (and fragkon.c:342-363 for the k-mer tool)
 *
 * i.e. "decode one alignment, filter it, tally it".  A caller now hands *blocks of raw
 * BAM alignment records* (exactly the bytes between two record boundaries of an
 * inflated BAM stream) to pssbam_engine_submit*, and collects the same two
 * unsigned long[(N+2)][16] tables (pss-bam.c:24-35, :755-756) and/or the two k-mer
 * tables (fragkon.c:335-336) from pssbam_engine_finish.
 *
 * Plain C types only.  Every function returns 0 on success and a negative PSSBAM_E*
 * code on failure; pssbam_last_error() then describes it.  The library never calls
 * exit() and never falls back to a CPU implementation: without a usable gfx950 device
 * pssbam_engine_create fails with PSSBAM_ENODEV.
 *
 * Threading: an engine is owned by one host thread at a time; different engines
 * (e.g. one per GPU) are independent.  All work is issued on one HIP stream per engine.
 */
#ifndef PSSBAM_HIP_H
#define PSSBAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSSBAM_ABI_VERSION 1
#define PSSBAM_MAX_KLEN 15     /* 4^15 64-bit bins per k-mer table = 8.6 GB of device memory */
#define PSSBAM_MAX_READ_GROUPS 4096  /* pssbam_engine_set_read_groups */
#define PSSBAM_MAX_LENGTH_BINS 64    /* pssbam_engine_set_length_bins: at most 63 edges */
#define PSSBAM_MAX_CONTIG_SETS 4096  /* pssbam_engine_set_contig_sets */
#define PSSBAM_MAX_REPLICATES 64     /* pssbam_engine_set_replicates */
#define PSSBAM_MAX_MISMATCHES 255    /* pssbam_engine_set_mismatches: the largest histogram limit and the largest filter limit */
#define PSSBAM_MAX_INTERIOR_MARGIN 65535 /* pssbam_engine_set_interior: the largest margin */
#define PSSBAM_MAX_COMPOSITION 30    /* pssbam_engine_set_composition: the largest width */
#define PSSBAM_MAX_SCORE_DIST 64     /* pssbam_engine_set_read_score: the most distance rows of the weight table */
#define PSSBAM_MAX_SCORE_QUAL 64     /* pssbam_engine_set_read_score: the most quality columns of the weight table */
#define PSSBAM_MAX_SCORE_WEIGHT 2047 /* pssbam_engine_set_read_score: the largest weight, either sign */
#define PSSBAM_MAX_SCORE_HALF 128    /* pssbam_engine_set_read_score: the largest half width of the score histogram */
#define PSSBAM_MAX_HIST_LENGTH 65535 /* pssbam_engine_set_length_histogram: the largest limit (lengths above it share one row) */
#define PSSBAM_MAX_BASE_QUALITY 93   /* pssbam_engine_set_min_base_quality: the largest Phred value SAM text can print */
#define PSSBAM_MAX_REGIONS (1 << 26) /* pssbam_engine_set_regions: intervals in one call */
#define PSSBAM_SITE_NONE 0           /* pssbam_engine_set_site_context: off */
#define PSSBAM_SITE_CPG 1            /* ... the reference position lies in a CpG dinucleotide */
#define PSSBAM_MAX_END_DEPTH 8       /* pssbam_engine_set_end_condition: positions of an end that are searched for its mark */
#define PSSBAM_END_MASK_OFF 0        /* pssbam_engine_set_end_mask: the sinks' records are the input's, byte for byte */
#define PSSBAM_END_MASK_ALL 1        /* ... every base of the two end regions becomes N */
#define PSSBAM_END_MASK_DS 2         /* ... only T in the 5' and A in the 3' region, in the read's orientation */
#define PSSBAM_END_MASK_SS 3         /* ... only T in either region, in the read's orientation */
#define PSSBAM_MAX_END_MASK 65535    /* pssbam_engine_set_end_mask: the widest region */

/* error codes */
#define PSSBAM_OK 0
#define PSSBAM_EINVAL (-1)   /* bad argument / option outside the supported range        */
#define PSSBAM_ENODEV (-2)   /* no gfx950 device, or the HIP runtime refused to start    */
#define PSSBAM_EHIP (-3)     /* a HIP call failed (message has the HIP error string)     */
#define PSSBAM_ENOMEM (-4)
#define PSSBAM_ESTATE (-5)   /* call order violated (e.g. submit before set_genome)      */
#define PSSBAM_EFORMAT (-6)  /* malformed record block                                   */
#define PSSBAM_EBUSY (-7)    /* pssbam_engine_submit_bgzf before the genome: every feed slot is full; set the genome first */

/* which tallies one pass produces */
#define PSSBAM_TALLY_PSS 1u   /* substitution tables, pss-bam.c process_aln              */
#define PSSBAM_TALLY_KMER 2u  /* fragmentation-point k-mers, fragkon.c process_aln       */

/* kernel selection (diagnostics / tests; 0 lets the engine choose) */
#define PSSBAM_KERNEL_AUTO 0
#define PSSBAM_KERNEL_SIMPLE 1  /* lane-per-read, global gathers: the cross-check kernel  */
#define PSSBAM_KERNEL_TILED 2   /* LDS-staged record prefixes, lane=row tally; 32 table   */
                                /* rows per pass over the block (what AUTO picks)         */

/* pss-bam's option globals, /root/reference/pss-bam.c:12-18 (set by -r -l -L -q -U -D -m) */
typedef struct pssbam_pss_opts {
    int32_t region_len;        /* REGION_LEN, >= 0                                       */
    uint64_t min_read_len;     /* MIN_READ_LEN                                           */
    uint64_t max_read_len;     /* MAX_READ_LEN                                           */
    int32_t min_mq;            /* MIN_MQ (compared unsigned, as the reference does)      */
    const char *up_ctx;        /* UP_CTX: set of allowed first upstream bases            */
    const char *down_ctx;      /* DOWN_CTX                                               */
    int32_t merged_only;       /* MERGED_ONLY                                            */
} pssbam_pss_opts;

/* fragkon's option globals, /root/reference/fragkon.c:14-18 (set by -k -l -L -q -m) */
typedef struct pssbam_kmer_opts {
    int32_t klen;              /* KLEN, 1..PSSBAM_MAX_KLEN on the device                 */
    int32_t min_mq;
    uint64_t min_read_len;
    uint64_t max_read_len;
    int32_t merged_only;
} pssbam_kmer_opts;

typedef struct pssbam_config {
    uint32_t abi_version;      /* PSSBAM_ABI_VERSION                                     */
    uint32_t tally_mask;       /* PSSBAM_TALLY_*                                         */
    pssbam_pss_opts pss;       /* read when PSSBAM_TALLY_PSS is set                      */
    pssbam_kmer_opts kmer;     /* read when PSSBAM_TALLY_KMER is set                     */
    const char *read_group;    /* -R: keep only records with RG:Z:<this>; NULL = all
                                  (replaces `samtools view -r`, pss-bam.c:150-155)       */
    int32_t device;            /* HIP device ordinal, -1 = current device                */
    int32_t kernel;            /* PSSBAM_KERNEL_*                                        */
} pssbam_config;

typedef struct pssbam_engine pssbam_engine; /* opaque */
struct genome;                              /* Genome of fasta-genome-io.h               */

/* indices into the stats[] array of pssbam_engine_finish */
enum {
    PSSBAM_ST_RECORDS = 0,     /* records submitted                                      */
    PSSBAM_ST_RG_DROPPED = 1,  /* removed by the -R filter (never reach line2saml)       */
    PSSBAM_ST_PARSE_SKIP = 2,  /* line2saml would return 1 (SEQ/QUAL length mismatch)    */
    PSSBAM_ST_NO_CONTIG = 3,   /* find_seq fails: process_aln returns 1                  */
    PSSBAM_ST_PSS_OK = 4,      /* pss process_aln returns 0                              */
    PSSBAM_ST_PSS_FILTERED = 5,/* pss process_aln returns -1                             */
    PSSBAM_ST_KMER_OK = 6,     /* fragkon process_aln returns 0                          */
    PSSBAM_ST_KMER_FILTERED = 7,/* fragkon process_aln returns 2                         */
    PSSBAM_ST_KMER_FAIL = 8,   /* fragkon process_aln returns -1 (non-ACGT in a k-mer)   */
    PSSBAM_ST_SLOW_PATH = 9,   /* diagnostics: records the tiled kernel had to read from
                                  global memory (needed prefix larger than what it stages) */
    PSSBAM_ST_N = 16
};

const char *pssbam_last_error(void);      /* thread-local, never NULL                    */
int pssbam_device_count(void);            /* number of usable gfx950 devices, 0 if none  */
/* Optional: brings the HIP runtime and the device's context up (tens of ms) so that a caller
 * can overlap it with its own start-up work, e.g. from a helper thread while the FASTA loads
 * (nothing in the reference corresponds; pssbam_engine_create does it otherwise). */
int pssbam_warmup(int device);

int pssbam_engine_create(const pssbam_config *cfg, pssbam_engine **out);
void pssbam_engine_destroy(pssbam_engine *e);

/* Adopt an existing hipStream_t (e.g. torch's current stream) instead of the engine's
 * own.  Call before any submit. */
int pssbam_engine_set_stream(pssbam_engine *e, void *hip_stream);

/* Uploads the reference bases (1 byte per base, upper case as loaded, each contig
 * followed by zero padding) and remembers the sorted id table so contig lookup has
 * find_seq's strcmp semantics (fasta-genome-io.c:202-219).  The Genome stays owned by
 * the caller and may be destroyed afterwards. */
int pssbam_engine_set_genome(pssbam_engine *e, const struct genome *g);
/* The same without the wait: returns once the upload is enqueued (copies, case folding and 4-bit packing
 * run on a stream of their own; tally launches wait for them on the device), so one host thread can start
 * the uploads of several GPUs at once and the engine's stream keeps inflating meanwhile.  The Genome must
 * stay untouched until pssbam_engine_genome_wait, _sync or _finish has returned.  The reference loads the
 * genome, then loops (pss-bam.c:751-783); this is what lets the replacement overlap the two.
 * The one exception to "one thread per engine": after pssbam_engine_feed_open, set_genome_async may be called
 * from ANOTHER thread while the owning thread keeps submitting compressed blocks, provided set_references
 * follows on the owning thread after set_genome_async has returned. */
int pssbam_engine_set_genome_async(pssbam_engine *e, const struct genome *g);
int pssbam_engine_genome_wait(pssbam_engine *e);

/* Same from plain arrays; when seqs_on_device != 0 the seqs[i] are device pointers
 * (bench / generators) and are copied device-to-device. */
int pssbam_engine_set_genome_arrays(pssbam_engine *e, size_t n, const char *const *ids,
                                    const uint8_t *const *seqs, const uint64_t *lens,
                                    int seqs_on_device);

/* The BAM header's reference list, in refID order.  Each name is looked up in the
 * genome exactly like find_seq(genome, RNAME) would be for that record's text form. */
int pssbam_engine_set_references(pssbam_engine *e, int32_t n_ref, const char *const *names);

/* One block of whole BAM alignment records (each = le32 block_size + block_size
 * bytes), nbytes < 4 GiB.  offsets[i] is the byte offset of record i's block_size
 * word, offsets[n_records] == nbytes.  Host memory; the engine has copied what it
 * needs when the call returns (the copy and the kernel run asynchronously). */
int pssbam_engine_submit(pssbam_engine *e, const void *records, uint64_t nbytes,
                         const uint32_t *offsets, uint32_t n_records);

/* The same without the wait: returns as soon as the copy and the kernel are enqueued, so that one
 * host thread can keep the PCIe links of several GPUs busy at once (one engine per GPU).  The
 * caller's buffers must stay untouched until pssbam_engine_wait_copied(e, *ticket) has returned
 * (or pssbam_engine_copy_done says 1, or the engine has been synced).  *ticket == 0: nothing was
 * in flight (empty block).  Replaces nothing in the reference (its loop is synchronous,
 * pss-bam.c:764-783); pssbam_engine_submit == submit_async + wait_copied. */
int pssbam_engine_submit_async(pssbam_engine *e, const void *records, uint64_t nbytes,
                               const uint32_t *offsets, uint32_t n_records, uint64_t *ticket);
int pssbam_engine_wait_copied(pssbam_engine *e, uint64_t ticket);
int pssbam_engine_copy_done(pssbam_engine *e, uint64_t ticket);   /* 1 done, 0 in flight, < 0 error */

/* Same with both arrays already resident in device memory; nothing is copied and the
 * buffers must stay valid until pssbam_engine_sync / finish.  d_records must be 16-byte
 * aligned and readable up to nbytes rounded up to 16 (any hipMalloc / torch allocation is). */
int pssbam_engine_submit_device(pssbam_engine *e, const void *d_records, uint64_t nbytes,
                                const uint32_t *d_offsets, uint32_t n_records);

int pssbam_engine_sync(pssbam_engine *e);

/* Drains the stream and copies the accumulated tables out.  Any pointer may be NULL.
 *   fwd, rev : (region_len+2)*16 each; row 0/1 = 2nd/1st context base, row 2+i = position i
 *   k5, k3   : 4^klen each (64-bit; the fragkon front end clamps to UINT_MAX on print,
 *              kmer.c:102-104)
 * Tables keep accumulating across calls until pssbam_engine_reset. */
int pssbam_engine_finish(pssbam_engine *e, unsigned long *fwd, unsigned long *rev, uint64_t *k5,
                         uint64_t *k3, uint64_t stats[PSSBAM_ST_N]);
int pssbam_engine_reset(pssbam_engine *e);

/* Read groups (pss-bam -G): one set of substitution tables per @RG ID in a single pass over the records,
 * instead of one `-R <ID>` run per library.  ids[0..n-1] are the header's IDs in order, n in
 * 1..PSSBAM_MAX_READ_GROUPS; an ID given twice keeps its first index.  A record belongs to ID g when its FIRST
 * RG:Z aux field equals ids[g] byte for byte -- exactly the records `-R ids[g]` keeps -- and to the unassigned
 * bucket otherwise (no RG:Z, or a value no ID matches).  Legal after create (or reset) and before the first
 * tally launch; with pssbam_engine_feed_open that is any time before set_references.  PSSBAM_EINVAL with
 * cfg.read_group set or with PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER together, PSSBAM_ESTATE once records have been tallied or the counter block
 * has been bound.  The table survives pssbam_engine_reset.  pssbam_engine_finish keeps returning the totals
 * over every record. */
int pssbam_engine_set_read_groups(pssbam_engine *e, int32_t n, const char *const *ids);
/* Drains the engine like pssbam_engine_finish and copies one group's two tables ((region_len+2)*16 each, any
 * pointer may be NULL): group -1 is the unassigned bucket, 0..n-1 the IDs in the order given.  With length bins
 * (below) group k is bin k and group -1 is all zeros.  With contig sets (below) group s is set s and group -1
 * holds the records on contigs no set lists.  With replicates (below) group j is replicate j and group -1 is all
 * zeros. */
int pssbam_engine_finish_groups(pssbam_engine *e, int32_t group, unsigned long *fwd, unsigned long *rev);

/* K-mer planes (fragkon -G / -S / -C).  An engine whose tally_mask is PSSBAM_TALLY_KMER alone takes the three
 * setters as well, one at a time and under the same ordering rules; each plane is then one [k5 | k3] pair of 4^klen
 * bins instead of a pair of substitution tables.  Read groups and contig sets pick the plane as above.  Length
 * bins go by the length fragkon's -l / -L compare, the SEQ length for paired reads too (not |TLEN|), and their
 * edges are checked against cfg.kmer.min_read_len / max_read_len: bin k holds what `fragkon -l <bin start>
 * -L <bin end>` tallies.  The 5' and the 3' add of one record go to the same plane, each on its own.  The counter
 * block grows by n planes of 2 * 4^klen words; when that does not fit the device's free memory the setter returns
 * PSSBAM_ENOMEM.  pssbam_engine_finish keeps returning the totals over every plane and the status counters of the
 * same engine without planes.  With PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER together every setter stays PSSBAM_EINVAL.
 *
 * Drains the engine like pssbam_engine_finish and copies one plane's two tables (4^klen each, either pointer may
 * be NULL): group -1 is plane 0 (the unassigned bucket; all zeros with length bins), 0..n-1 as for
 * pssbam_engine_finish_groups.  PSSBAM_EINVAL on an engine that tallies substitution tables, as
 * pssbam_engine_finish_groups is on a k-mer engine. */
int pssbam_engine_finish_kmer_groups(pssbam_engine *e, int32_t group, uint64_t *k5, uint64_t *k3);

/* Length bins (pss-bam -S): one set of substitution tables per fragment-length bin in a single pass over the
 * records, instead of one `-l <lo> -L <hi>` run per window.  edges[0..n_edges-1], n_edges in
 * 1..PSSBAM_MAX_LENGTH_BINS-1, must rise strictly with cfg.pss.min_read_len < edges[0] and
 * edges[n_edges-1] <= cfg.pss.max_read_len.  Bin k is [edges[k-1], edges[k]-1], bin 0 starts at min_read_len and
 * bin n_edges ends at max_read_len: a record that passes every filter lands in bin #{edges <= its length}, the
 * length -l / -L compare (|TLEN| for paired reads, else the SEQ length), so bin k holds exactly what
 * `-l <bin start> -L <bin end>` tallies.  Legal after create (or reset) and before the first tally launch, like
 * pssbam_engine_set_read_groups, and allowed with cfg.read_group (bins of one read group).  PSSBAM_EINVAL with
 * PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER together, with read groups set or with bad edges, PSSBAM_ESTATE once records have been tallied or the
 * counter block has been bound.  The bins survive pssbam_engine_reset; pssbam_engine_finish keeps returning the
 * totals over every bin, pssbam_engine_finish_groups(e, k, ...) returns bin k. */
int pssbam_engine_set_length_bins(pssbam_engine *e, int32_t n_edges, const uint32_t *edges);

/* Contig sets (pss-bam -C): one set of substitution tables per set of reference sequences in a single pass over
 * the records, instead of one run per set with a FASTA cut down to that set's contigs.  names[0..n_names-1] are
 * contig names, set_of[i] in 0..n_sets-1 the set of names[i], n_sets in 1..PSSBAM_MAX_CONTIG_SETS; a name given
 * twice under the same set counts once, under two sets it is PSSBAM_EINVAL.  A record belongs to set s when its
 * RNAME (the @SQ name of its refID, "*" for refID -1) is listed under s -- exactly the records the reference
 * tallies with -F holding only s's contigs, since it skips every read whose RNAME find_seq cannot find -- and
 * to the unassigned bucket otherwise.  The engine keeps the name -> set map and applies it to every reference
 * table, so the call is legal before and after set_references (a later set_references, e.g. of the SAM-text
 * reader as new RNAMEs show up, applies it again).  Otherwise legal and illegal as
 * pssbam_engine_set_read_groups: after create (or reset) and before the first tally launch, allowed with
 * cfg.read_group; PSSBAM_EINVAL with PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER together, with read groups or length bins set, or with bad
 * arguments, PSSBAM_ESTATE once records have been tallied or the counter block has been bound.  The sets
 * survive pssbam_engine_reset; pssbam_engine_finish keeps returning the totals over every record,
 * pssbam_engine_finish_groups(e, s, ...) returns set s. */
int pssbam_engine_set_contig_sets(pssbam_engine *e, int32_t n_sets, int64_t n_names, const char *const *names,
                                  const int32_t *set_of);

/* Read-name replicates (pss-bam -J): K sets of substitution tables, each over a random K-th of the reads, in a single
 * pass over the records -- the planes a delete-one-group jackknife needs, instead of K runs on K hand-made subsets.
 * k = K in 2..PSSBAM_MAX_REPLICATES; k = 0 switches the setting off, and the engine then launches exactly the kernels
 * it launches without it.  The replicate of a record is a hash of its read name: with n = l_read_name - 1 (0 when
 * l_read_name <= 1) and b[0..n) the name bytes as stored from record offset 36 on (an embedded NUL is a byte like any
 * other),
 *     h = 2166136261
 *     for i = 0, 4, 8, ... < n:  h = (h ^ (b[i] | b[i+1] << 8 | b[i+2] << 16 | b[i+3] << 24)) * 16777619   (b[>= n] = 0)
 *     h ^= n;  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16              (all mod 2^32)
 *     replicate = (uint64(h) * K) >> 32
 * ("" -> h = 0xab3e7c0b, "a" -> 0x2a681819, "read/1" -> 0x9d5b3ad0, "r0000000" -> 0x4620f828).  Mates share a name and
 * so a replicate.  Replicate j is plane 1 + j and receives exactly what the same engine tallies on the input reduced
 * to the records of replicate j; plane 0 stays empty, as with length bins, and the counter block is the length-bin
 * layout with K planes: [fwd | rev | stats | fwd_0 | rev_0 | ... | fwd_K-1 | rev_K-1], summed across engines as one u64
 * array.  pssbam_engine_finish keeps returning the totals over every record and the status counters of the engine
 * without the setting; pssbam_engine_finish_groups(e, j, ...) returns replicate j, group -1 all zeros.  Legal after
 * create (or reset) and before the first tally launch (after pssbam_engine_feed_open: before set_references); goes
 * with cfg.read_group, a minimum base quality and regions.  PSSBAM_EINVAL for k = 1 or outside 0..64, with
 * PSSBAM_TALLY_KMER in the mask, and with read groups, length bins, contig sets, per-contig tables, a length histogram,
 * site context, an end condition, gapped reads or the mismatch count set (those setters return PSSBAM_EINVAL, "... and
 * replicates exclude each other", once this one is on); PSSBAM_ESTATE once records have been tallied or the counter
 * block has been bound.  The setting survives pssbam_engine_reset. */
int pssbam_engine_set_replicates(pssbam_engine *e, int32_t k);

/* Per-contig tables (pss-bam -A): every reference sequence's own pair of substitution tables in a single pass over the
 * records, for any number of references (a metagenomic BAM has 10^4 .. 10^6), without a map file.  Plane k belongs to
 * refID k, k in 0..n_ref-1 of the table pssbam_engine_set_references gives, and plane n_ref to the refID -1 records
 * (RNAME "*"); plane k receives exactly what the ordinary tables receive from the records whose refID is k, so for a
 * header of distinct names it equals pssbam_engine_set_contig_sets with the one set {name k} and the reference run with
 * a FASTA that holds only contig k.  Two refIDs that carry the same name keep separate planes.  The totals
 * (pssbam_engine_finish, the sum of all planes) and the status counters are those of the engine without the setting.
 * The counter block is [fwd | rev | stats | fwd_0 | rev_0 | ... | fwd_nref | rev_nref | touched_0 .. touched_nref]:
 * the leading pair stays zero, plane k lies (k * 2 * (region_len + 2) * 16) words behind the stats -- 64-bit offsets --
 * and touched_k is non-zero exactly when plane k holds a non-zero word, so a reader of the block need not walk empty
 * planes; the block still sums across engines as one u64 array.  pssbam_engine_finish_groups(e, k, ...) returns plane
 * k.  The block is sized when the reference count is known: at pssbam_engine_set_references, or from
 * pssbam_engine_feed_open's n_ref; a later set_references with another count re-sizes it (once records have been
 * tallied the count may only grow -- the SAM-text reader -- and the planes keep their contents).  PSSBAM_ENOMEM when
 * (n_ref + 1) * 2 * (region_len + 2) * 16 words do not fit the device's free memory.  on == 0 switches the setting off:
 * the engine then launches exactly the kernels it launches without it.  Legal after create (or reset) and before the
 * first tally launch (after pssbam_engine_feed_open: before set_references); goes with cfg.read_group, a minimum base
 * quality and regions.  PSSBAM_EINVAL with PSSBAM_TALLY_KMER in the mask and with read groups, length bins, contig sets,
 * a length histogram, site context, an end condition or gapped reads set (those setters return PSSBAM_EINVAL once this
 * one is on); PSSBAM_ESTATE once records have been tallied or the counter block has been bound, and from
 * set_references when a bound block would have to change size.  The setting survives pssbam_engine_reset. */
int pssbam_engine_set_per_contig(pssbam_engine *e, int32_t on);

/* Planes first_ref .. first_ref + n - 1 of a per-contig engine (plane n_ref: refID -1), drained like
 * pssbam_engine_finish: fwd and rev take n * (region_len + 2) * 16 words each, touched[i] = 1 when plane first_ref + i
 * holds a non-zero word (an untouched plane is returned as zeros and is not read back from the device).  Any pointer
 * may be NULL.  PSSBAM_ESTATE without pssbam_engine_set_per_contig, PSSBAM_EINVAL for a range outside 0..n_ref. */
int pssbam_engine_finish_contigs(pssbam_engine *e, int32_t first_ref, int32_t n, unsigned long *fwd, unsigned long *rev,
                                 uint8_t *touched);

/* Minimum base quality (pss-bam -Q): read bases whose quality is below q are left out of the substitution tables,
 * as the tools that estimate damage from such tables do (a sequencing error at a Q2-Q15 base is no substitution).
 * q is a Phred value -- the BAM QUAL byte, the SAM character - 33 -- in 0..PSSBAM_MAX_BASE_QUALITY; 0 switches
 * the mask off and the engine then launches exactly the kernels it launches without this call.  For q > 0
 * interior position i (0..region_len-1) of an alignment end adds nothing to its table when the QUAL byte of the
 * read base it pairs with (base i for the left end, base L-1-i for the right end, on either strand) is < q.  That
 * is what the reference does with a read base that is not A/C/G/T (add_fwd_counts / add_rev_counts skip it), and
 * nothing else of it looks at the content of SEQ, so
 *     the tables with minimum base quality q == the tables without it on the same records with every SEQ base
 *     whose quality is below q replaced by 'N'.
 * Rows 0 and 1 (the context bases) are reference-only and never masked.  The record filters, -U / -D, the plane a
 * record falls in and every status counter stay as they are: a read whose window is masked entirely still counts
 * as PSSBAM_ST_PSS_OK.  Absent qualities (0xFF fill) compare as 255 and mask nothing.  The k-mer tables of a
 * PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER engine are unaffected.  The tiled kernels stage whole records for q > 0
 * (QUAL lies behind SEQ), as they do with cfg.read_group.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time
 * before set_references.  Goes with cfg.read_group and with each of read groups, length bins and contig sets.
 * PSSBAM_EINVAL for q outside the range or on an engine without PSSBAM_TALLY_PSS, PSSBAM_ESTATE once records have
 * been tallied.  The value survives pssbam_engine_reset.  The counter block keeps its layout; engines whose blocks
 * are summed (pssbam_reduce_counters, a caller's RCCL reduce) must all have been given the same q. */
int pssbam_engine_set_min_base_quality(pssbam_engine *e, int32_t q);

/* Regions (pss-bam -T, fragkon -T): only records whose alignment overlaps an interval of a BED-style list are
 * tallied, so that
 *     the tables with regions == the tables without them on the input reduced to the records that
 *     `samtools view -L regions.bed` keeps.
 * A record's alignment is [POS-1, POS-1 + reference length of its CIGAR); only a record whose CIGAR is exactly <L>M
 * can be tallied by either tool, so for every candidate that is [pos, pos + L).  Interval i is the 0-based half-open
 * [starts[i], ends[i]) on contig names[name_of[i]], name_of[i] in 0..n_names-1.  A read that ends at a start or
 * starts at an end does not overlap; one shared base does.  Context bases and k-mer windows outside the alignment
 * play no part.  Intervals may come in any order and may overlap, nest or touch: the engine sorts them per contig
 * and merges them.  start > end is PSSBAM_EINVAL, start == end an empty interval that is dropped, an end beyond the
 * contig is clamped.  A name given twice is the same contig; names are matched to the @SQ name of the record's refID
 * exactly as pssbam_engine_set_contig_sets matches them, and a name no reference carries has no effect.  A contig
 * that is not listed, or is left without an interval, tallies nothing.
 * It is one more record filter: a candidate that meets no region counts as PSSBAM_ST_PSS_FILTERED /
 * PSSBAM_ST_KMER_FILTERED; RECORDS, RG_DROPPED, PARSE_SKIP and NO_CONTIG stay as without regions.  It picks no plane,
 * so it goes with cfg.read_group, with each of read groups, length bins and contig sets (every plane is what its
 * single run gives with the same regions), with a minimum base quality and with both tally masks, alone or together.
 * n_regions == 0 switches the filter off: the engine then launches exactly the kernels it launches without this
 * call.  The engine keeps the name -> intervals map and packs the device table whenever set_references or this call
 * arrives, so the call is legal before and after set_references.  Legal after create (or reset) and before the first
 * tally launch; with pssbam_engine_feed_open that is any time before set_references.  PSSBAM_ESTATE once records have
 * been tallied, PSSBAM_ENOMEM when the table does not fit the device.  The regions survive pssbam_engine_reset.  The
 * counter block keeps its layout; engines whose blocks are summed (pssbam_reduce_counters, a caller's RCCL reduce)
 * must all have been given the same regions.  $PSSBAM_REGION_GRID_SHIFT (2..20, default 10) sets the bases per word
 * of the lookup grid (2^shift). */
int pssbam_engine_set_regions(pssbam_engine *e, int32_t n_names, const char *const *names, int64_t n_regions,
                              const int32_t *name_of, const uint32_t *starts, const uint32_t *ends);

/* Fragment-length histogram (pss-bam -H) of the reads that are added to the substitution tables, counted in the
 * tally kernel itself from the registers that hold a read's length and fate: no second pass, no extra bytes read.
 * With limit max_len = M (1..PSSBAM_MAX_HIST_LENGTH; 0 switches the histogram off and the engine then launches
 * exactly the kernels it launches without this call) the engine keeps two arrays of M + 2 counters, hf and hr.  For
 * every record let L be the length -l / -L compare -- |TLEN| of a paired read, else the length of the SEQ text -- and
 * b = min(L, M + 1): hf[b] += 1 when the record is added to the forward table, hr[b] += 1 when it is added to the
 * reverse table.  An unpaired read that passes counts in both, a paired one in one; row M + 1 collects every longer
 * read.  Every filter that decides "added" shapes the histogram as it shapes the tables (flags, the <L>M CIGAR rule,
 * -q, -l / -L, -m, -U / -D, the contig-edge test, cfg.read_group, regions); a minimum base quality masks bases, not
 * reads, and changes nothing.  So with OK(x..y) = PSSBAM_ST_PSS_OK of the same options run with -l x -L y (cut to the
 * run's own -l / -L): on unpaired records hf[l] == hr[l] == OK(l..l); on any input hf[l] + hr[l] ==
 * 2 * OK_unpaired(l..l) + OK_paired(l..l).  The tables, the status counters and the k-mer tables of a
 * PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER engine stay bit-identical.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time
 * before set_references.  Goes with cfg.read_group, a minimum base quality, regions and both tally masks together.
 * PSSBAM_EINVAL for max_len outside the range, on an engine without PSSBAM_TALLY_PSS, and with read groups, length
 * bins or contig sets set (those setters return PSSBAM_EINVAL once the histogram is on: one histogram per plane is
 * not kept); PSSBAM_ESTATE once records have been tallied or the counter block has been bound (the block grows, see
 * pssbam_engine_counters_device).  The setting survives pssbam_engine_reset; engines whose blocks are summed must all
 * have been given the same limit. */
int pssbam_engine_set_length_histogram(pssbam_engine *e, int32_t max_len);

/* Drains the engine like pssbam_engine_finish and copies the two arrays, max_len + 2 words each; either pointer may
 * be NULL.  PSSBAM_EINVAL when the histogram is off. */
int pssbam_engine_finish_length_histogram(pssbam_engine *e, uint64_t *fwd, uint64_t *rev);

/* Site context (pss-bam -X cpg): a second pair of substitution tables, IN, over the interior positions whose REFERENCE
 * position lies in a given context, from the same pass as the ordinary tables T.  With g the contig's bases after the
 * case folding the engine applies anyway, position p is in CpG context (PSSBAM_SITE_CPG) when
 *     (g[p] == 'C' && g[p+1] == 'G') || (g[p] == 'G' && g[p-1] == 'C');
 * a neighbour outside the contig counts as "no" (every position a tallied read touches has both inside).  The set is
 * its own reverse complement and is evaluated in genome orientation for reads of both strands.  Interior position i
 * of an alignment end adds to IN exactly when it adds to T and the reference position it pairs with -- POS-1+i for the
 * left end, POS-1+L-1-i for the right end, on either strand -- is in context.  Rows 0 and 1 (the context bases) are
 * reference-only and never masked: IN returns T's.  Nothing of the reference looks at the content of SEQ except
 * add_fwd_counts / add_rev_counts, which skip a read base that is not A/C/G/T, so
 *     IN == the tables of the same records with SEQ base k set to 'N' wherever contig position POS-1+k is NOT in
 *     context, and T - IN on rows 2+ (rows 0/1 as T) == the same with the complementary mask.
 * T, every status counter and the record filters are bit-identical to the engine without the setting; a base masked
 * by a minimum base quality is missing from T and from IN alike.  PSSBAM_SITE_NONE switches it off: the engine then
 * launches exactly the kernels it launches without this call.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time
 * before set_references.  Goes with cfg.read_group, a minimum base quality and regions.  PSSBAM_EINVAL for an unknown
 * mode, on an engine with PSSBAM_TALLY_KMER in its mask, and with read groups, length bins, contig sets or a length
 * histogram set (those setters return PSSBAM_EINVAL once site context is on); PSSBAM_ESTATE once records have been
 * tallied or the counter block has been bound (the block grows, see pssbam_engine_counters_device).  The setting
 * survives pssbam_engine_reset; engines whose blocks are summed must all have been given the same mode. */
int pssbam_engine_set_site_context(pssbam_engine *e, int32_t mode);

/* Drains the engine like pssbam_engine_finish and copies IN's two tables, (region_len+2)*16 words each with rows 0/1
 * filled from T; either pointer may be NULL.  PSSBAM_EINVAL when the setting is off. */
int pssbam_engine_finish_site_context(pssbam_engine *e, unsigned long *fwd_in, unsigned long *rev_in);

/* End condition (pss-bam -E): a second pair of substitution tables, COND, over the unpaired records whose OTHER end
 * carries a given substitution, from the same pass as the ordinary tables T -- the conditional substitution analysis
 * of damage (a fragment with a C->T at its 5' end is almost certainly old, so the 3' table over those fragments alone
 * measures damage in a contaminated library).  For a record that is added to the tables let o[0..L-1] / g[0..L-1] be
 * the read and reference bases as process_aln pairs them (upper case, both reverse-complemented for a FLAG 0x10 read):
 * forward-table row 2+i receives (o[i], g[i]), reverse-table row 2+i receives (o[L-1-i], g[L-1-i]), and
 * cell(r, f) = 4*code(r) + code(f) with A 0, C 1, G 2, T 3 is the column of the counts file; a pair with a member that
 * is not A/C/G/T has no cell.  With depth d (1..PSSBAM_MAX_END_DEPTH, d <= region_len) and the cells cell5, cell3
 * (0..15; 13 = read T on reference C, 2 = read A on reference G) a record is
 *     5'-marked when it is unpaired (FLAG 0x1 clear) and cell(o[i], g[i]) == cell5 for some i < d,
 *     3'-marked when it is unpaired and cell(o[L-1-i], g[L-1-i]) == cell3 for some i < d.
 * A base below a minimum base quality has no cell (it behaves as N, as pssbam_engine_set_min_base_quality states).  A
 * tallied read has L >= region_len >= d, so every position looked at exists; the two windows may overlap (L < 2d).
 * COND.fwd receives a record's whole forward contribution (rows 0 and 1 included) exactly when the record is added to
 * T.fwd, is unpaired and is 3'-marked; COND.rev its whole reverse contribution exactly when it is added to T.rev, is
 * unpaired and is 5'-marked.  Paired records never reach COND: their other end lives in another record.  Four read
 * counters go with the pair: reads[0] = unpaired records added to the tables, reads[1] = those that are 5'-marked,
 * reads[2] = those that are 3'-marked, reads[3] = those that are both.  So
 *     COND.fwd == the forward table of the same options on the input reduced to the unpaired 3'-marked records,
 *     COND.rev == the reverse table on the input reduced to the unpaired 5'-marked records,
 * and T, every status counter and the record filters are bit-identical to the engine without the setting.  depth == 0
 * switches it off: the engine then launches exactly the kernels it launches without this call and n_u64 is unchanged.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time
 * before set_references.  Goes with cfg.read_group, a minimum base quality and regions.  PSSBAM_EINVAL for arguments
 * outside their ranges, for depth > region_len, for region_len > 30 (the marks are taken from the code words of the
 * one 32-row pass that holds both ends' first positions; a later pass of a larger -r would have to gather them
 * again, so it is refused), on an engine with PSSBAM_TALLY_KMER in its mask, and with read groups, length bins, contig
 * sets, a length histogram or site context set (those setters return PSSBAM_EINVAL once the end condition is on);
 * PSSBAM_ESTATE once records have been tallied or the counter block has been bound (the block grows, see
 * pssbam_engine_counters_device).  The setting survives pssbam_engine_reset; engines whose blocks are summed must all
 * have been given the same arguments. */
int pssbam_engine_set_end_condition(pssbam_engine *e, int32_t depth, int32_t cell5, int32_t cell3);

/* Drains the engine like pssbam_engine_finish and copies COND's two tables, (region_len+2)*16 words each, and the four
 * read counters; any pointer may be NULL.  PSSBAM_EINVAL when the setting is off. */
int pssbam_engine_finish_end_condition(pssbam_engine *e, unsigned long *fwd_c, unsigned long *rev_c, uint64_t reads[4]);

/* pss-bam -I: clipped and gapped reads are tallied by their anchored ends (on != 0; 0 switches it off again).  A record
 * ANCHORS when
 *   1. its CIGAR has at least one op and every op length is >= 1;
 *   2. it reads [H][S] core [S][H] -- at most one hard clip at either extreme, at most one soft clip inside it
 *      (lengths clipL / clipR, else 0) -- and the core is non-empty, holds only M I D = X, and starts and ends with a
 *      match-type op (M, = or X); an N, a P, an interior clip or a core that starts or ends with I / D: no anchor;
 *   3. SEQ and QUAL are present and clipL + (M I = X of the core) + clipR == l_seq;
 *   4. span = (M D = X of the core) <= 2^31 - 1.
 * With a / b the summed lengths of the match-type runs at the core's start / end (a = b = span when the core has no
 * I / D), the tables and status counters are those of the engine without the setting on the records in which every
 * anchoring record has been replaced by the one that differs from it in
 *     CIGAR = <span>M,
 *     SEQ'  = SEQ[clipL, clipL + a) + "N" * (span - a - b) + SEQ[l_seq - clipR - b, l_seq - clipR)
 *             (SEQ[clipL, l_seq - clipR) when the core is all match-type),
 *     QUAL' sliced the same way with Phred 0 as filler;
 * a record that does not anchor is treated as without the setting, and a <len>M record anchors to itself.  So both
 * ends sit where the reference has them, the length that min_read_len / max_read_len and region_len compare is the
 * span of an unpaired read (a paired one still needs |TLEN| == span), and a position counts when no I / D lies between
 * it and one of the alignment's two ends and adds nothing otherwise, like an N.
 * PSSBAM_ST_SLOW_PATH alone may differ: a record of more than 16 CIGAR ops, and a gapped record whose every I / D lies
 * within region_len reference bases of one end, takes the tiled kernels' one-lane path.
 * The counter block keeps its size and layout (a bound block stays bound) and there is no new status slot.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time
 * before set_references.  Goes with cfg.read_group, a minimum base quality and regions.  PSSBAM_EINVAL on an engine
 * with PSSBAM_TALLY_KMER in its mask and with read groups, length bins, contig sets, a length histogram, site context
 * or an end condition set (those setters return PSSBAM_EINVAL once this one is on); PSSBAM_ESTATE once records have
 * been tallied.  The setting survives pssbam_engine_reset; engines whose blocks are summed must all have it. */
int pssbam_engine_set_gapped_reads(pssbam_engine *e, int32_t on);

/* Mismatch count (pss-bam -n / -N / -V): a record filter on the number of mismatches between the whole read and the
 * reference, and the histogram of that number over the reads that are added to the tables, from the same pass.
 * The mismatch count m of a record is defined for a record whose CIGAR is exactly <L>M, L being the length that
 * min_read_len / max_read_len compare, on a contig the genome holds.  With seq[i] read base i as stored (the BAM nibble),
 * g[p] the contig after the case folding the engine applies anyway and s = POS - 1:
 *     m = #{ i in [0, min(L, l_seq)) : seq[i] in {A,C,G,T}, g[s+i] in {A,C,G,T}, seq[i] != g[s+i] }
 * and with transversions_only the unordered pair {seq[i], g[s+i]} must also be neither {A,G} nor {C,T}.  Nothing else
 * counts: N, IUPAC codes and '=' in the read, any non-ACGT reference base, bases at or beyond l_seq.  m is the same for
 * both strands (complementing both bases keeps inequality and the transition / transversion class), is taken from SEQ as
 * stored -- a minimum base quality masks table positions and does not change m -- and is a full 32-bit count: a
 * 300-base read that differs everywhere has m = 300.
 * Filter, max_mismatches = k (0..PSSBAM_MAX_MISMATCHES; -1 = off): one more record filter, like regions.  A record that
 * every other filter would add to a table and that has m > k counts as PSSBAM_ST_PSS_FILTERED; RECORDS, RG_DROPPED,
 * PARSE_SKIP, NO_CONTIG and the sum PSS_OK + PSS_FILTERED stay as without the setting.  With RED(k) the input without
 * the <L>M records on known contigs whose m exceeds k: fwd, rev and PSS_OK == those of the engine without the setting
 * on RED(k) with the same options.
 * Histogram, hist_max = M (1..PSSBAM_MAX_MISMATCHES; 0 = off): two arrays of M + 2 counters, mf and mr.  With
 * b = min(m, M + 1): mf[b] += 1 when the record is added to the forward table, mr[b] += 1 when it is added to the
 * reverse table.  These are the identities of the length histogram with "the input reduced to the records whose
 * min(m, M + 1) equals b" in place of "-l b -L b": unpaired records give mf[b] == mr[b] == OK(b); on any input
 * mf[b] + mr[b] == 2 * OK_unpaired(b) + OK_paired(b).  With the filter on only kept reads are counted, so rows above k
 * are zero.  Tables and status counters are bit-identical to the engine without the histogram.
 * (0, -1, x) switches everything off: the engine then launches exactly the kernels it launches without this call and
 * n_u64 is unchanged.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time
 * before set_references.  Goes with cfg.read_group, a minimum base quality and regions.  PSSBAM_EINVAL for arguments
 * outside their ranges, on an engine with PSSBAM_TALLY_KMER in its mask, for region_len > 30 (the decision is taken in
 * the one pass that holds all rows, as for the end condition), and with read groups, length bins, contig sets, a length
 * histogram, site context, an end condition, gapped reads or per-contig tables set (each of those setters returns
 * PSSBAM_EINVAL once this one is on); PSSBAM_ESTATE once records have been tallied, or once a bound counter block would
 * have to grow (see pssbam_engine_counters_device).  The setting survives pssbam_engine_reset; engines whose blocks are
 * summed must all have been given the same three arguments. */
int pssbam_engine_set_mismatches(pssbam_engine *e, int32_t hist_max /*0 = no histogram*/,
                                 int32_t max_mismatches /*-1 = no filter*/, int32_t transversions_only);

/* Drains the engine like pssbam_engine_finish and copies the two arrays, hist_max + 2 words each; either pointer may
 * be NULL.  PSSBAM_EINVAL without a histogram. */
int pssbam_engine_finish_mismatches(pssbam_engine *e, uint64_t *fwd, uint64_t *rev);

/* Interior table (pss-bam -W): the 4 x 4 substitution table of the read interior, every read position at least `margin` bases
 * from both ends of its read, from the same pass -- the sequencing-error and polymorphism background that the end rows are
 * read against.  Take a record that is added to the forward or to the reverse table after every record filter the run has
 * (flags, mapping quality, lengths, merged_only, the read group, regions, the contig and edge checks, the mate rules, and
 * up_ctx / down_ctx as they decide today).  With L the length that min_read_len / max_read_len compare, g the contig after the
 * case folding, s = POS - 1, seq[i] the stored BAM nibble and d = margin, the record's interior is
 *     I = { i : d <= i, i + d < L, i < l_seq }
 * and position i of I counts when seq[i] and g[s+i] are both one of A C G T and, with a minimum base quality q, QUAL[i] >= q
 * (absent qualities, 0xFF, mask nothing).  With rd / rf the codes A0 C1 G2 T3 of read and reference base it counts into
 * table[4*rd + rf] for a forward-strand record and into table[15 - (4*rd + rf)] for a reverse-strand one (both bases
 * complemented: the read's orientation, like the tables).  N, IUPAC codes and '=' in the read, any other reference letter
 * and bases at or beyond l_seq never count.  reads = the number of such records whose I is not empty.  A record that goes
 * into one table only (a read 1, a read 2) counts once, a
 * record that enters neither does not count.  d is independent of region_len; d = 0 is the table of the whole read.  For
 * unpaired <x>M records this is, per length x, the sum of rows d .. x-d-1 of the forward table of a run with
 * min_read_len = max_read_len = x and region_len = x - d.
 * margin = 0..PSSBAM_MAX_INTERIOR_MARGIN; -1 switches the setting off: the engine then launches exactly the kernels it
 * launches without this call and n_u64 is unchanged.  Tables and status counters are bit-identical to the engine without
 * the setting.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time before
 * set_references.  Goes with cfg.read_group, a minimum base quality and regions.  PSSBAM_EINVAL for a margin out of range, on
 * an engine whose mask is not PSSBAM_TALLY_PSS alone, for region_len > 30 (a read's fate is decided in the one pass that
 * holds all rows, as for the mismatch count), and with read groups, length bins, contig sets, per-contig tables,
 * replicates, a length histogram, site context, an end condition, gapped reads or the mismatch count set (each of those
 * setters returns PSSBAM_EINVAL once this one is on); PSSBAM_ESTATE once records have been tallied, or once a bound counter
 * block would have to grow (see pssbam_engine_counters_device).  The setting survives pssbam_engine_reset; engines whose
 * blocks are summed must all have been given the same margin.  PSSBAM_KERNEL_AUTO never takes tally_compact with it on. */
int pssbam_engine_set_interior(pssbam_engine *e, int32_t margin /*-1 = off*/);

/* Drains the engine like pssbam_engine_finish and copies table[16] and reads; either pointer may be NULL.  PSSBAM_EINVAL
 * when the setting is off. */
int pssbam_engine_finish_interior(pssbam_engine *e, uint64_t table[16], uint64_t *reads);

/* Composition table (pss-bam -P): the reference base composition in a window of `width` = w bases on either side of the two
 * fragmentation points, outside and inside the read, in the read's orientation, from the same pass -- the depurination
 * signal (purine excess at -1, C depletion at +1) against its own baseline further out.  Take a record that is added to the
 * forward table, to the reverse table, or to both, after every record filter the run has (flags, the <L>M CIGAR, mapping
 * quality, lengths, merged_only, the read group, regions, the contig and edge checks, the mate rules, and up_ctx / down_ctx
 * as they decide today).  With L the length that min_read_len / max_read_len compare, s = POS - 1, len the contig's length,
 * g the contig after the case folding, cls(x) = 0 1 2 3 for A C G T and 4 for anything else, and comp(c) = 3 - c for
 * c < 4, comp(4) = 4: for every offset j in -w .. w-1 (negative: outside the read, -1 adjacent to it; 0 ..: inside, counted
 * from that end)
 *   5' block, for a record added to the forward table: p = s + j on a forward-strand record, p = s + L-1 - j on a FLAG 0x10
 *             record; adds 1 to c5[j + w][c];
 *   3' block, for a record added to the reverse table: p = s + L-1 - j on a forward-strand record, p = s + j on a FLAG 0x10
 *             record; adds 1 to c3[j + w][c];
 *   c = cls(g[p]), on a FLAG 0x10 record comp(cls(g[p])).
 * A position counts only when 0 <= p < len, and for j >= 0 only when j < L (L >= region_len is all that is guaranteed, and
 * w is independent of region_len).  Positions are masked by their coordinate, not by their letter: nothing of the
 * padding between contigs or of a neighbouring contig is ever counted.  SEQ and QUAL play no part, so a minimum base quality
 * changes nothing; an unpaired read counts in both blocks, a read 1 in the 5' block only, a read 2 in the 3' block only.
 * c5[w-1] and c5[w-2] are the diagonal cells of the forward table's context rows -1 and -2, c3[w-1] and c3[w-2] those of
 * the reverse table's.
 * width = 1..PSSBAM_MAX_COMPOSITION; 0 switches the setting off: the engine then launches exactly the kernels it launches
 * without this call and n_u64 is unchanged.  Tables and status counters are bit-identical to the engine without the
 * setting.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time before
 * set_references.  Goes with cfg.read_group, regions and a minimum base quality (which has no effect).  PSSBAM_EINVAL for a
 * width out of range, on an engine whose mask is not PSSBAM_TALLY_PSS alone, for region_len > 30 (a read's fate and its end
 * windows are those of the one pass that holds all rows, as for the interior table), and with read groups, length bins,
 * contig sets, per-contig tables, replicates, a length histogram, site context, an end condition, gapped reads, the
 * mismatch count or the interior table set (each of those setters returns PSSBAM_EINVAL once this one is on);
 * PSSBAM_ESTATE once records have been tallied, or once a bound counter block would have to grow (see
 * pssbam_engine_counters_device).  The setting survives pssbam_engine_reset; engines whose blocks are summed must all have
 * been given the same width.  PSSBAM_KERNEL_AUTO never takes tally_compact with it on. */
int pssbam_engine_set_composition(pssbam_engine *e, int32_t width /*0 = off*/);

/* Drains the engine like pssbam_engine_finish and copies c5 and c3, 2 * width * 5 words each, row-major [j + width][class];
 * either pointer may be NULL.  PSSBAM_EINVAL when the setting is off. */
int pssbam_engine_finish_composition(pssbam_engine *e, uint64_t *c5, uint64_t *c3);

/* Read score (pss-bam -y / -Y): a record filter on a sum of caller-supplied integer weights over the C and G sites of the whole
 * read, and the histogram of that sum over the reads that are added to the tables, from the same pass.  The engine knows
 * nothing of what the weights mean; pss-bam passes the log-likelihood ratios of a post-mortem-damage model.
 * The score S of a record is defined for the records the mismatch count is defined for: a CIGAR of exactly <L>M, L being the
 * length that min_read_len / max_read_len compare, on a contig the genome holds.  With s = POS - 1, seq[i] read base i as stored
 * (the BAM nibble), g[p] the contig after the case folding the engine applies anyway and rev = FLAG 0x10, position
 * i < min(L, l_seq) takes part when s + i lies inside the contig, seq[i] and g[s+i] are both one of A C G T and -- with a minimum
 * base quality set -- QUAL[i] >= min_bq (the rule of the interior table: absent qualities, 0xFF, are never below).  A position that
 * takes part contributes weights[kind][d][q]:
 *     g = C, seq = C:  d = min(i, n_dist-1),        kind 0 on a forward read, 2 on a reverse read
 *     g = C, seq = T:  d = min(i, n_dist-1),        kind 1 / 3
 *     g = G, seq = G:  d = min(L-1-i, n_dist-1),    kind 2 / 0
 *     g = G, seq = A:  d = min(L-1-i, n_dist-1),    kind 3 / 1
 *     anything else:   nothing
 * q = min(QUAL[i], n_qual-1) on the stored byte, so absent qualities land in the last column.  In read orientation kinds 0 / 1
 * are C->C and C->T by distance from the 5' end, kinds 2 / 3 G->G and G->A by distance from the 3' end.  S is the mathematical
 * sum clamped to the int32 range (with |w| <= PSSBAM_MAX_SCORE_WEIGHT 32 bits cannot overflow below 2^20 bases).
 * weights: int16 [4][n_dist][n_qual], n_dist = 1..PSSBAM_MAX_SCORE_DIST, n_qual = 1..PSSBAM_MAX_SCORE_QUAL, every entry within
 * +-PSSBAM_MAX_SCORE_WEIGHT; copied to the device at the call.  NULL switches everything off (the other arguments are then
 * ignored): the engine then launches exactly the kernels it launches without this call and n_u64 is unchanged.
 * Filter, use_filter != 0: one more record filter, like the mismatch limit.  A record that every other filter would add to a
 * table and that has S < min_score counts as PSSBAM_ST_PSS_FILTERED; RECORDS, RG_DROPPED, PARSE_SKIP, NO_CONTIG and the sum
 * PSS_OK + PSS_FILTERED stay as without the setting.  fwd, rev and PSS_OK == those of the engine without the setting on the input
 * without the records whose S is defined and below min_score.
 * Histogram, hist_half = H (1..PSSBAM_MAX_SCORE_HALF; 0 = off), hist_shift = 0..16: two arrays of 2H counters, sf and sr.  With
 * b = clamp(S >> hist_shift, -H, H-1) + H, the shift arithmetic (it floors negative scores too): sf[b] += 1 when the record is
 * added to the forward table, sr[b] += 1 when it is added to the reverse table -- the identities of the mismatch histogram with
 * "the records whose bin is b".  With the filter on only kept reads are counted.  Tables and status counters are bit-identical to
 * the engine without the histogram.
 * Legal after create (or reset) and before the first tally launch; with pssbam_engine_feed_open that is any time before
 * set_references.  Goes with cfg.read_group, a minimum base quality and regions.  PSSBAM_EINVAL for arguments outside their
 * ranges or a weight beyond the limit, on an engine whose mask is not PSSBAM_TALLY_PSS alone, for region_len > 30 (the decision is
 * taken in the one pass that holds all rows), and with read groups, length bins, contig sets, per-contig tables, replicates, a
 * length histogram, site context, an end condition, gapped reads, the mismatch count, the interior table or the composition
 * table set (each of those setters returns PSSBAM_EINVAL once this one is on); PSSBAM_ESTATE once records have been tallied, or
 * once a bound counter block would have to grow (see pssbam_engine_counters_device).  The setting survives pssbam_engine_reset;
 * engines whose blocks are summed must all have been given the same arguments.  PSSBAM_KERNEL_AUTO never takes tally_compact
 * with it on. */
int pssbam_engine_set_read_score(pssbam_engine *e, const int16_t *weights /*[4][n_dist][n_qual], NULL = off*/, int32_t n_dist,
                                 int32_t n_qual, int32_t use_filter, int32_t min_score, int32_t hist_half /*0 = no histogram*/,
                                 int32_t hist_shift /*0..16*/);

/* The record sink (pss-bam -O): besides tallying them, the engine hands over the alignment records that were added to the
 * forward or the reverse main table -- the records for which PSSBAM_ST_PSS_OK counts, after every filter of the run (cfg.pss,
 * cfg.read_group, regions, gapped reads, the mismatch limit, the read score's minimum; each mate on its own; a minimum base
 * quality masks bases and drops no record, except through the score).  The sink receives whole records (le32 block_size +
 * body) back to back, byte-identical to the input (unless an end mask is set: pssbam_engine_set_end_mask) and in input order
 * across all submits, n_records of them in nbytes bytes;
 * the memory is valid during the call only.  It is called on the thread that calls the engine and nowhere else, from inside
 * the submit functions, pssbam_engine_sync, _finish and _reset: every submit delivers the chunks whose copy to the host has
 * completed, sync / finish / reset deliver everything outstanding before they return.  A block none of whose records is kept
 * delivers nothing.  A non-zero return makes the engine call fail with PSSBAM_EINVAL, and the sink is not called again.  The call
 * that fails is always in a clean state: a submit fails at its top, before anything of it is queued (its block has NOT been
 * tallied and may be submitted again); sync / finish / reset fail after everything else they do is done (calling them again
 * succeeds).  A chunk that arrives while a submit is already queuing its kernels is handed over there, but a failure of the sink
 * on it is reported by the next engine call of the kinds above -- the block of that submit is tallied, and launches that were put
 * off for the genome all go on.  The tallies go on after a failure; only the hand-over stops.
 * The engine starts no thread for it.
 * The selection runs on the device behind the tally kernels of each block (three steps: mark, prefix sum, gather) and its
 * output crosses to the host beside the next block's kernels; tables, status counters and the launch count of
 * pssbam_engine_kernel_time are those of the run without a sink.  Without a sink the engine allocates and launches
 * nothing for it.  Blocks given to an engine with a sink hold at most 2^32 - 256 bytes.
 * Legal before the first submit after create or reset (PSSBAM_ESTATE otherwise); sink = NULL switches it off.  PSSBAM_EINVAL
 * on an engine without PSSBAM_TALLY_PSS.  The setting survives pssbam_engine_reset.  Engines are independent: the order
 * across the engines of a multi-GPU run is the caller's business. */
typedef int (*pssbam_record_sink)(void *ctx, const void *records, uint64_t nbytes, uint64_t n_records);
int pssbam_engine_set_record_sink(pssbam_engine *e, pssbam_record_sink sink, void *ctx);

/* The block sink (pss-bam -O ... -Z): the record sink's stream, deflated on the device.  The records the record sink would
 * receive are cut into BGZF payloads of 0xFF00 bytes at fixed offsets of each chunk (records may cross blocks, as in files
 * written by htsjdk), every payload becomes one complete BGZF block on the device (csrc/deflate_kernels.h: dynamic-Huffman
 * DEFLATE over LZ77 matches, or stored where that is not smaller; CRC-32 and ISIZE included), and the blocks cross to the
 * host packed back to back.  The sink receives a whole number of complete blocks: n_blocks of them in nbytes bytes, which
 * inflate to raw_bytes bytes holding n_records whole records.  Concatenated over all calls they inflate to exactly the byte
 * stream the record sink would have delivered for the same input and settings.  The compressed bytes depend on the input
 * AND on how it was cut into submits -- each chunk closes its last block, so a different cut moves the block boundaries --
 * while the inflated stream does not depend on the cut.  The same input in the same submits gives the same bytes on every
 * run.  No EOF block is delivered: the stream's end is the caller's to mark.
 * Everything else is as for pssbam_engine_set_record_sink: which records are kept, the thread that calls the sink, the
 * calls that deliver (every submit delivers the chunks whose copy to the host has completed; sync / finish / reset deliver
 * everything outstanding), a chunk with no kept record delivers nothing, a non-zero return makes the engine call fail with
 * PSSBAM_EINVAL in the same clean states and the sink is not called again, the tallies go on.  Tables, status counters and
 * the time and launch count of pssbam_engine_kernel_time are those of the run without a sink; without a block sink nothing
 * is allocated or launched for it (three more kernels behind the gather -- deflate, and the pack's scan and copy --, one
 * strided buffer of 64 KiB per block, a length and an offset per block otherwise; under pssbam_engine_feed_open they come out of the feed's memory budget).  Legal before the first
 * submit after create or reset (PSSBAM_ESTATE otherwise); sink = NULL switches it off; PSSBAM_EINVAL on an engine without
 * PSSBAM_TALLY_PSS and while a record sink is set (pssbam_engine_set_record_sink likewise returns PSSBAM_EINVAL while a
 * block sink is set: one or the other).  The setting survives pssbam_engine_reset. */
typedef int (*pssbam_block_sink)(void *ctx, const void *bgzf, uint64_t nbytes, uint64_t n_blocks, uint64_t raw_bytes,
                                 uint64_t n_records);
int pssbam_engine_set_block_sink(pssbam_engine *e, pssbam_block_sink sink, void *ctx);

/* The end mask (pss-bam -K): the records a sink receives are the input's except at their masked positions, where the 4-bit
 * SEQ code is 15 (N) and the QUAL byte 0; nothing else of a record changes, no length, and neither which records are kept nor
 * their order.  With l = l_seq, rev = flag & 0x10 and i the 0-based index into SEQ as stored, the 5' region is i < min(n5, l)
 * on a forward read and i >= l - min(n5, l) on a reverse one, the 3' region i >= l - min(n3, l) and i < min(n3, l).
 * PSSBAM_END_MASK_ALL masks every position of either region; PSSBAM_END_MASK_DS (double-stranded library: C->T from the 5',
 * G->A from the 3' end) the positions of the 5' region whose stored code is T (8) on a forward and A (1) on a reverse read and
 * those of the 3' region whose stored code is A on a forward and T on a reverse read; PSSBAM_END_MASK_SS (C->T at both ends) the
 * positions of either region whose stored code is T on a forward and A on a reverse read.  A position of both regions is
 * masked when either rule masks it.  Soft-clipped bases are SEQ bases and count from the ends of SEQ; each mate goes by its own
 * 0x10.  When the first QUAL byte is 0xFF (no qualities) QUAL is left alone.  A record whose fields do not fit inside it
 * (36 + l_read_name + 4 * n_cigar_op + (l + 1) / 2 + l > 4 + block_size) goes out unchanged; no byte outside a record's own SEQ
 * and QUAL is ever written.
 * The mask acts on the sinks' copy alone, behind the tally and behind the selection (one more kernel between the gather and
 * the deflate, csrc/end_mask_kernels.h; no memory of its own): tables, status counters, the set of kept records and the time
 * and launch count of pssbam_engine_kernel_time are those of the run without it; a minimum base quality, the mismatch limit
 * and the read score judge the unmasked read.  The block sink's blocks deflate the masked stream.  Without a sink, and with
 * PSSBAM_END_MASK_OFF, it has no effect: nothing more is launched.  May be set before or after the sink.
 * Legal before the first submit after create or reset (PSSBAM_ESTATE otherwise).  PSSBAM_EINVAL for an unknown mode, for
 * n5 or n3 above PSSBAM_MAX_END_MASK, and for n5 == n3 == 0 with a mode other than PSSBAM_END_MASK_OFF.  The setting survives pssbam_engine_reset. */
int pssbam_engine_set_end_mask(pssbam_engine *e, int32_t mode, uint32_t n5, uint32_t n3);

/* Duplicate flagging (pss-bam -d, fragkon -d): with the setting on, a run equals the same run on the same input after the
 * duplicates, as defined here, have had FLAG bit 0x400 set.  The engine sets that bit in its device copy of every block, in front
 * of the block's tally kernels (csrc/dedup_kernels.h), so every other setting works on the deduplicated input unchanged: a flagged
 * record counts as PSSBAM_ST_PSS_FILTERED / _KMER_FILTERED and reaches no table, plane, histogram or sink.
 *   Input order: the order of the submit calls, and the record order inside each block.
 *   Eligible: an unpaired record (FLAG 0x1 clear) that is a candidate of the engine's tool -- not dropped by cfg.read_group, not a
 *     parse skip, contig known, none of 0x4 0x100 0x200 0x400 0x800, CIGAR exactly <L>M, the tool's mapping quality and length
 *     window, inside the contig by the tool's margin, and the regions when set.  What looks at the read's bases or at the reference
 *     (-U / -D contexts, a minimum base quality, the mismatch limit, the read score) takes no part: those filters apply after
 *     deduplication, so a group whose first record fails one of them contributes nothing.
 *   Key: (refID, POS, L, FLAG & 0x10, g); L = the SEQ length, g = with read groups (pssbam_engine_set_read_groups) 0 for the
 *     unassigned bucket and 1 + the group's index otherwise, without them 0: duplicates are per library.
 *   Duplicate: an eligible record with an earlier eligible record of the same key, in input order, across all blocks since create
 *     or reset.  The first record of a key wins (not the one with the best base qualities: that needs look-ahead across blocks).
 *     The result depends neither on how the input is cut into blocks, nor on its being sorted, nor on GPU scheduling.
 *   Paired and ineligible records are never flagged and shadow nothing; records that arrive flagged 0x400 stay flagged and count
 *     nowhere.  Pairing mates is out of scope.
 * on != 0 switches it on; initial_slots is the first size of the key table, rounded up to a power of two (0 = the engine's default;
 * the table doubles as the run needs, PSSBAM_ENOMEM from the submit that cannot grow it).  Legal after create or reset and before
 * the first submit (with pssbam_engine_feed_open: before the first submit_bgzf), PSSBAM_ESTATE later.  It goes with every other
 * setting except gapped reads (pssbam_engine_set_gapped_reads): PSSBAM_EINVAL in either order of the two calls, and on an engine
 * with PSSBAM_TALLY_PSS | PSSBAM_TALLY_KMER together, whose two eligibilities differ.  The counter block keeps its size and layout,
 * and the time and launch count of pssbam_engine_kernel_time stay the tally's.  The setting survives pssbam_engine_reset, which
 * empties the table.  Engines do not share a table.  Off, nothing is allocated and nothing more is launched.
 * With pssbam_engine_submit_device the device copy is the caller's: the engine sets bit 0x400 of the duplicates' FLAG in the
 * caller's buffer.  A caller who needs the bytes unchanged uses pssbam_engine_submit. */
#define PSSBAM_MAX_DUP_HIST 65535
int pssbam_engine_set_duplicates(pssbam_engine *e, int32_t on, uint32_t initial_slots);
/* Drains like pssbam_engine_finish.  totals = {eligible records, distinct keys, records flagged = eligible - distinct};
 * hist[c], c in 1..hist_max: keys with exactly c eligible records; hist[hist_max+1]: keys with more; hist[0] = 0;
 * hist_max+2 words, hist may be NULL.  PSSBAM_EINVAL when the setting is off. */
int pssbam_engine_finish_duplicates(pssbam_engine *e, uint64_t totals[3], uint64_t *hist, int32_t hist_max);

/* Depth of coverage of the kept records (pss-bam -c / -b), from the same pass.
 *   Kept: exactly the records a record sink delivers -- added to the forward or the reverse main table of this run, after every
 *     filter given (read group, mapping quality, lengths, merged only, contexts, regions, the mismatch limit, the read score, and the
 *     0x400 bits duplicate flagging sets).  Each mate of a pair is judged on its own.
 *   depth(c, p) = the kept records on contig c with POS <= p < POS + L; L = the record's length in the tables, which for a kept record
 *     is the length of its <L>M CIGAR (and of its SEQ, unless a paired record's SEQ disagrees with its CIGAR and TLEN).  Mates that
 *     overlap count twice.  A minimum base quality masks bases, not reads, and the end mask changes the sink's bytes only: neither
 *     changes the depth.
 * The engine keeps one uint32_t per stored genome position (4 bytes per base: 12.4 GB for a human genome) holding differences; behind
 * each block's tally kernels one more kernel adds the kept records' two entries each (csrc/coverage_kernels.h).  Depth is exact below
 * 2^32.  The counter block keeps its size and layout, and the time and launch count of pssbam_engine_kernel_time stay the tally's.
 * on != 0 switches it on; positions_hint = the positions the genome is expected to have (the sum of the BAM header's LN values; 0 =
 * unknown): with pssbam_engine_feed_open, 4 x positions_hint plus the contigs' padding is left out of the feed's memory budget.  The
 * array is allocated when the genome's size is known -- by this call when the genome is set already, by set_genome otherwise --
 * and PSSBAM_ENOMEM comes from the call that cannot get it.  Legal after create or reset and before the first submit (with
 * pssbam_engine_feed_open: before the first submit_bgzf), PSSBAM_ESTATE later.  PSSBAM_EINVAL without PSSBAM_TALLY_PSS, and with
 * gapped reads (pssbam_engine_set_gapped_reads) in either order of the two calls: the span of a clipped or gapped read needs a
 * definition of its own.  The setting survives pssbam_engine_reset, which zeroes the array at the size it has.  Engines do not share
 * an array, and pssbam_reduce_counters does not sum them.  Off, nothing is allocated and nothing more is launched. */
#define PSSBAM_COV_HIST_MAX 255
int pssbam_engine_set_coverage(pssbam_engine *e, int32_t on, uint64_t positions_hint);
/* Drains like pssbam_engine_finish, then computes the totals of everything submitted since create or reset.  Non-destructive: it may
 * be called any number of times, more blocks may follow it, and the depth array itself is never stored.
 *   per_contig: n x {covered positions, sum of depth, maximum depth} for the references first_ref .. first_ref + n - 1 of the last
 *     set_references (index n_ref = a contig named "*"); all zero for a name the genome lacks, and for the later one of two
 *     references of the same name.
 *   hist[d], d in 0..hist_max (at most PSSBAM_COV_HIST_MAX): the positions at depth d of the contigs of the reference list, each
 *     contig once; hist[hist_max + 1]: the positions above; hist_max + 2 words.  The padding between contigs counts nowhere.
 *   n_runs: the number of maximal runs of equal non-zero depth (pssbam_engine_finish_coverage_runs).
 * Any of the three pointers may be NULL.  PSSBAM_EINVAL when the setting is off. */
int pssbam_engine_finish_coverage(pssbam_engine *e, int32_t first_ref, int32_t n, uint64_t *per_contig, uint64_t *hist, int32_t hist_max,
                                  uint64_t *n_runs);
/* The covered intervals (a bedGraph): run i is the half-open interval [start[i], end[i]) of reference ref[i] (-1: the contig named
 * "*") at depth[i] > 0.  Runs are maximal (a run ends where the depth changes, and only there: two runs that touch differ in depth),
 * ordered by refID, then start, and never cross a contig.  *n_runs = the exact count, always; with all four arrays NULL that is
 * all the call does.  Any single array may be NULL.  PSSBAM_EINVAL when cap, the room of each array, is below the count, and when
 * the setting is off.  Called behind pssbam_engine_finish_coverage with nothing submitted in between, it starts from that call's
 * tile sums instead of computing them again. */
int pssbam_engine_finish_coverage_runs(pssbam_engine *e, uint64_t cap, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *depth,
                                       uint64_t *n_runs);
/* Fixed windows (pss-bam -w): every reference of the last set_references that the genome holds is cut into the windows
 * [k * window, min((k + 1) * window, length)), k = 0 .. ceil(length / window) - 1, contig-relative and 0-based; the last window of a
 * contig may be short, none crosses a contig, and padding belongs to none.  Window i is [start[i], end[i]) of reference ref[i] (-1:
 * the contig named "*"); acgt[i] = its positions whose FASTA letter, upper-cased, is A, C, G or T; gc[i] = those that are C or G;
 * covered[i] = its positions at depth > 0; depth_sum[i] = the sum of depth(c, p) over it, depth as defined above.  All exact.  Windows
 * come by refID, then start; the later one of two references of the same name has none.  *n_windows = the exact count, always;
 * with all seven arrays NULL that is all the call does.  Any single array may be NULL.  Drains like pssbam_engine_finish_coverage, is
 * non-destructive and may be called any number of times; it starts from the tile sums of an earlier finish call when nothing was
 * submitted since, and keeps its own result for the same window until a block is submitted, the references or the genome change,
 * the engine is reset or coverage is switched off.  The accumulators (20 bytes per window, in up to 64 copies while that stays below 1.3 MB) are allocated by the call and freed by
 * it: PSSBAM_ENOMEM when they do not fit the device.  PSSBAM_EINVAL for a window outside PSSBAM_COV_WINDOW_MIN ..
 * PSSBAM_COV_WINDOW_MAX, when the count does not fit 32 bits, when cap, the room of each array, is below the count, and when the
 * setting is off; PSSBAM_ESTATE without a genome and references.  Nothing is launched or allocated while the call is not used. */
#define PSSBAM_COV_WINDOW_MIN 16u
#define PSSBAM_COV_WINDOW_MAX (1u << 30)
int pssbam_engine_finish_coverage_windows(pssbam_engine *e, uint32_t window, uint64_t cap, int32_t *ref, uint32_t *start, uint32_t *end,
                                          uint32_t *acgt, uint32_t *gc, uint32_t *covered, uint64_t *depth_sum, uint64_t *n_windows);

/* Strand-split allele counts of the kept records at listed sites (pss-bam -a / -t), from the same pass: the pileup at a SNP panel.
 *   A site is a (contig, 0-based position) pair: site i is pos0[i] on the contig named names[name_of[i]].  Positions may come in any
 *     order; duplicates are merged.  Names are matched to the names of pssbam_engine_set_references exactly as
 *     pssbam_engine_set_regions matches them: a name no reference carries is dropped, so is a position at or beyond the contig's
 *     stored length, and so is the later of two references of the same name.  The engine keeps the name -> positions map and
 *     packs the device table whenever this call or set_references arrives.
 *   Kept: exactly the records a record sink delivers and the coverage counts (above), each mate on its own.
 *   A kept record with start s and table length L (the length of its <L>M CIGAR) shows, at every resolved site p of its contig with
 *     s + trim <= p < s + L - trim, the stored SEQ base at offset p - s; a record with 2 * trim >= L shows nothing.  The site's counter
 *     [strand][code] goes up by one: strand 0 = forward, 1 = FLAG 0x10; code = A, C, G, T or other.  Other takes N and every IUPAC
 *     nibble, under a minimum base quality a base whose QUAL is below it (an absent QUAL, 0xFF, is never below), and an offset at or
 *     beyond l_seq (a paired record whose SEQ disagrees with its CIGAR).  With trim 0 the ten counters of a site sum to the depth of
 *     coverage there.  The end mask changes the sink's bytes only: the counts are of the unmasked read.
 * Device side (csrc/allele_kernels.h): the resolved sites as sorted 64-bit genome indices (8 bytes a site), a lookup grid of one
 * uint32_t per 2^shift genome positions ($PSSBAM_SITE_GRID_SHIFT, 2..20, default 10) and ten uint32_t counters a site, exact below
 * 2^32; one more kernel behind each block's tally kernels.  The counter block keeps its size and layout, and the time and launch
 * count of pssbam_engine_kernel_time stay the tally's.
 * n_sites == 0 switches it off.  Legal after create or reset, before or after set_references, and before the first submit
 * (PSSBAM_ESTATE later).  PSSBAM_EINVAL without PSSBAM_TALLY_PSS, with gapped reads (pssbam_engine_set_gapped_reads) in either order of
 * the two calls, for n_sites above PSSBAM_MAX_REGIONS and for trim above PSSBAM_MAX_SITE_TRIM; PSSBAM_ENOMEM from the call that cannot
 * get the memory.  The setting survives pssbam_engine_reset, which zeroes the counters.  Engines share nothing, and
 * pssbam_reduce_counters does not sum these counters.  Off, nothing is allocated and nothing more is launched. */
#define PSSBAM_MAX_SITE_TRIM 65535
int pssbam_engine_set_sites(pssbam_engine *e, int32_t n_names, const char *const *names, int64_t n_sites, const int32_t *name_of,
                            const uint32_t *pos0, uint32_t trim);
/* Drains like pssbam_engine_finish, then gives the counts of everything submitted since create or reset.  Non-destructive: it may be
 * called any number of times, and more blocks may follow.  The resolved sites come ordered by reference index, then
 * position: ref[i], pos0[i], ref_base[i] = the genome's stored base there as a letter (A C G T, anything else N;
 * gathered by a small kernel) and counts[10 * i ..] = fA fC fG fT fO rA rC rG rT rO.  *n_sites = the exact count, always; with the
 * four arrays and totals NULL that is all the call does.  Any single array may be NULL.  totals (may be NULL) = {sites given after
 * merging, sites resolved, sites with a non-zero sum, bases counted}.  PSSBAM_EINVAL when cap, the room of each array, is below the
 * count, and when the setting is off. */
int pssbam_engine_finish_sites(pssbam_engine *e, uint64_t cap, int32_t *ref, uint32_t *pos0, uint8_t *ref_base,
                               uint32_t *counts /* 10 per site: fA fC fG fT fO rA rC rG rT rO */, uint64_t *n_sites, uint64_t totals[4]);

/* Drains the engine like pssbam_engine_finish and copies the two arrays, 2 * hist_half words each; either pointer may be
 * NULL.  PSSBAM_EINVAL without a histogram. */
int pssbam_engine_finish_read_score(pssbam_engine *e, uint64_t *fwd, uint64_t *rev);

/* The device-resident counter block [fwd | rev | k5 | k3 | stats] as one array of
 * n_u64 64-bit words, for a caller-side RCCL reduce across GPUs (sum, uint64).  With read groups it is
 * [fwd | rev | stats | fwd_0 | rev_0 | ... | fwd_n-1 | rev_n-1]: the leading fwd | rev are the unassigned
 * bucket, group g's pair ((region_len+2)*16 words each) starts at 2*(region_len+2)*16 + PSSBAM_ST_N +
 * g*2*(region_len+2)*16 (a PSSBAM_TALLY_PSS engine has no k-mer tables).  With length bins the
 * layout is the same with bin k in group k's place, and the leading fwd | rev stay zero.  With contig sets it is
 * the same with set s in group s's place, the leading fwd | rev the records on unlisted contigs.  A k-mer engine
 * with planes holds [k5 | k3 | stats | k5_0 | k3_0 | ... | k5_n-1 | k3_n-1]: the leading pair is plane 0, plane g's
 * pair (4^klen words each) starts at 2*4^klen + PSSBAM_ST_N + g*2*4^klen -- offsets that pass 2^32 words at large
 * klen.  The block is still summed across GPUs as one u64 array.
 * With a length histogram of limit M (pssbam_engine_set_length_histogram; never together with planes) the two
 * arrays are appended: [fwd | rev | k5 | k3 | stats | hf | hr], hf at 2*(region_len+2)*16 + 2*4^klen + PSSBAM_ST_N
 * (no k-mer term on a PSSBAM_TALLY_PSS engine), hr M + 2 words behind it, n_u64 larger by 2*(M+2).
 * With site context (pssbam_engine_set_site_context; a PSSBAM_TALLY_PSS engine without planes or histogram) the
 * in-context pair is appended: [fwd | rev | stats | fwd_in | rev_in], fwd_in at 2*(region_len+2)*16 + PSSBAM_ST_N (the
 * old n_u64), rev_in (region_len+2)*16 words behind it, n_u64 larger by 2*(region_len+2)*16.  Rows 0 and 1 of the
 * pair stay zero on the device (pssbam_engine_finish_site_context fills them from fwd | rev), so the block still sums
 * across engines as one u64 array.
 * With an end condition (pssbam_engine_set_end_condition; a PSSBAM_TALLY_PSS engine without planes, histogram or site
 * context) the conditional pair and its read counters are appended: [fwd | rev | stats | fwd_c | rev_c | reads[4]],
 * fwd_c at 2*(region_len+2)*16 + PSSBAM_ST_N (the old n_u64), rev_c (region_len+2)*16 words behind it, reads[0..3]
 * behind that, n_u64 larger by 2*(region_len+2)*16 + 4.  Every word is a plain count, so the block still sums across
 * engines as one u64 array and the PSSBAM_ST_* slots stay where they are.
 * With a mismatch histogram of limit M (pssbam_engine_set_mismatches; a PSSBAM_TALLY_PSS engine without any of the above)
 * the two arrays are appended: [fwd | rev | stats | mf | mr], mf at 2*(region_len+2)*16 + PSSBAM_ST_N (the old n_u64), mr
 * M + 2 words behind it, n_u64 larger by 2*(M+2).  All words are plain counts: the block still sums as one u64 array.  The
 * filter alone adds no words.
 * With the interior table (pssbam_engine_set_interior; a PSSBAM_TALLY_PSS engine without any of the above) its 17 words are
 * appended in the same place: [fwd | rev | stats | table[16] | reads], table at 2*(region_len+2)*16 + PSSBAM_ST_N (the old
 * n_u64), n_u64 larger by 17.  All words are plain counts: the block still sums as one u64 array.
 * With the composition table of width w (pssbam_engine_set_composition; a PSSBAM_TALLY_PSS engine without any of the above)
 * its two blocks are appended in the same place: [fwd | rev | stats | c5 | c3], c5 at 2*(region_len+2)*16 + PSSBAM_ST_N (the
 * old n_u64), c3 10*w words behind it, each row-major [j + w][class], n_u64 larger by 20*w.  All words are plain counts: the
 * block still sums as one u64 array.
 * With a read-score histogram of half width H (pssbam_engine_set_read_score; a PSSBAM_TALLY_PSS engine without any of the above)
 * the two arrays are appended in the same place: [fwd | rev | stats | sf | sr], sf at 2*(region_len+2)*16 + PSSBAM_ST_N (the old
 * n_u64), sr 2H words behind it, n_u64 larger by 4H.  All words are plain counts: the block still sums as one u64 array.  The
 * filter alone adds no words. */
int pssbam_engine_counters_device(pssbam_engine *e, void **d_counters, size_t *n_u64);

/* Makes the engine accumulate into caller-owned device memory (n_u64 words, as reported
 * by pssbam_engine_counters_device, 8-byte aligned, zeroed by the caller) -- e.g. a
 * torch tensor that is then handed to torch.distributed / RCCL in place.  The current
 * counts are carried over.  NULL returns to the engine's own block. */
int pssbam_engine_bind_counters(pssbam_engine *e, void *d_counters, size_t n_u64);

/* genome-kmer-count (/root/reference/genome-kmer-count.c:56-79) on the uploaded genome: counts
 * every k-mer start of every contig (windows touching a non-ACGT base are not counted), k in
 * 1..PSSBAM_MAX_KLEN.  counts[4^k] in the same bin order as the fragkon tables.  Needs set_genome only. */
int pssbam_engine_genome_kmer_count(pssbam_engine *e, int klen, uint64_t *counts);

/* Node-level sum for one process driving several GPUs (one engine per device): adds the
 * counter blocks of engines[1..n-1] into engines[root] with ONE RCCL ncclReduce(sum,
 * uint64) per device inside a group call over xGMI (communicators from ncclCommInitAll,
 * librccl loaded on first use), after draining every engine's stream.  All engines must
 * have been created with identical options.  n == 1 is a no-op.  Blocks below 32 MiB (the pss
 * tables are 7 KB) are summed through the host instead -- n small copies and an add take
 * microseconds, a communicator over 8 GPUs takes seconds -- unless PSSBAM_REDUCE=rccl;
 * PSSBAM_REDUCE=host forces the host sum for any size. */
int pssbam_reduce_counters(pssbam_engine *const *engines, int n, int root);

/* Page-locks a host range (hipHostRegister) so pssbam_engine_submit's copies from it run as
 * true async DMA; the front ends register the BAM reader's batch buffer once. */
int pssbam_host_register(void *ptr, size_t bytes);
int pssbam_host_unregister(void *ptr);

/* HIP-event stopwatch on the engine's stream: begin records an event, end records a
 * second one, waits for it and returns the elapsed device time in milliseconds. */
int pssbam_engine_timer_begin(pssbam_engine *e);
int pssbam_engine_timer_end(pssbam_engine *e, float *ms);
/* Sum of the tally kernels' own durations (event pair around every launch) and their
 * number since the last call with reset != 0. */
int pssbam_engine_kernel_time(pssbam_engine *e, double *total_ms, uint64_t *n_launches, int reset);

/* Drains the engine and reports where its device time went: summed H2D copy durations (events on
 * the copy stream) and bytes, summed tally-kernel durations and launches.  Any pointer may be NULL. */
int pssbam_engine_phase_times(pssbam_engine *e, double *h2d_ms, uint64_t *h2d_bytes, double *kernel_ms,
                              uint64_t *n_launches);

/* ---- device-side BGZF inflate (second half) --------------------------------------
 * What it replaces: the `samtools view` child that decompresses the BAM for the reference
 * (/root/reference/pss-bam.c:148-162) -- here the compressed file crosses PCIe and every BGZF
 * block (SAM spec 4.1; raw DEFLATE, RFC 1951) is inflated on the GPU, one lane per block. */
typedef struct pssbam_bgzf_block {
    uint64_t in_off;   /* offset of the block's raw deflate payload in the compressed buffer   */
    uint32_t in_len;   /* payload bytes                                                        */
    uint32_t isize;    /* ISIZE: bytes the block inflates to (<= 65536)                        */
    uint64_t out_off;  /* where they go in the output buffer                                   */
    uint32_t crc;      /* CRC-32 of the inflated bytes, from the block trailer                 */
    uint32_t status;   /* out: 0 = ok, else which check failed (1..8, csrc/inflate_kernels.h)  */
} pssbam_bgzf_block;

/* Walks the BGZF headers of bytes[0..nbytes): fills blocks[] (out_off = running sum of ISIZE) up to
 * max_blocks (blocks == NULL: count only), stops at the first partial block.  Returns the number
 * of whole blocks or PSSBAM_EFORMAT; *consumed = bytes they cover, *inflated_bytes = sum of ISIZE. */
int64_t pssbam_bgzf_scan(const void *bytes, uint64_t nbytes, pssbam_bgzf_block *blocks, uint64_t max_blocks,
                         uint64_t *consumed, uint64_t *inflated_bytes);

/* Inflates n_blocks blocks on the current device, asynchronously on hip_stream: d_comp (4-byte
 * aligned, readable 4 bytes past comp_bytes) -> d_out at each block's out_off; d_blocks[i].status
 * tells how block i went (check_crc != 0 adds the ISIZE/CRC-32 kernel).  d_out must hold
 * out_off + isize bytes for every block: the table is the caller's, and only its in_off / in_len /
 * isize are checked on the device (a block that fails them gets status 1 and is not touched). */
int pssbam_bgzf_inflate_device(void *hip_stream, const void *d_comp, uint64_t comp_bytes, pssbam_bgzf_block *d_blocks,
                               uint32_t n_blocks, void *d_out, int check_crc);

/* The whole feed in one call: a batch of whole BGZF blocks (compressed bytes in host memory,
 * page-locked for full PCIe speed; blocks[] from pssbam_bgzf_scan with in_off relative to comp and
 * out_off starting at 0, inflating to < 4 GiB) is copied, inflated, CRC-checked, record-indexed and
 * tallied on the device, asynchronously.  Consecutive calls continue ONE record stream (records may
 * cross BGZF blocks and calls); first_record_offset = bytes of the stream's first block that come
 * before the first alignment record (the BAM header; only in the first call after create / reset).
 * comp must stay untouched until pssbam_engine_wait_bgzf_copied(e, *ticket).  Whether the blocks
 * were sound is known once the work has run: pssbam_engine_feed_status. */
int pssbam_engine_submit_bgzf(pssbam_engine *e, const void *comp, uint64_t comp_bytes, const pssbam_bgzf_block *blocks,
                              uint32_t n_blocks, uint32_t first_record_offset, uint64_t *ticket);
int pssbam_engine_wait_bgzf_copied(pssbam_engine *e, uint64_t ticket);
/* Optional, BEFORE set_genome: declares that compressed blocks will be fed ahead of the genome.  n_ref = the
 * reference count of the BAM header (the record chain is judged with it; set_references must bring the same
 * count later).  pssbam_engine_submit_bgzf is then legal at once: inflate, CRC-32 and record index run as the
 * blocks arrive -- they need no reference base -- and the tally launches of every super-batch follow when
 * set_genome(_async) + set_references have been called.  The inflated records wait in device memory meanwhile
 * (a ring of 4.4 GB slots that grows within what the device has free, genome_bytes_hint -- e.g. the FASTA's
 * size, 0 = unknown -- left alone); when every slot is full submit_bgzf returns PSSBAM_EBUSY and has taken
 * NOTHING of that chunk: set the genome, then submit the chunk again. */
int pssbam_engine_feed_open(pssbam_engine *e, int32_t n_ref, uint64_t genome_bytes_hint);
/* The blocks submitted next do NOT continue the stream fed so far (an engine that is dealt every n-th
 * run of a file): pending blocks are processed, a partial record left at this point raises
 * PSSBAM_FEED_TRUNCATED, and the next blocks start a new record chain at their first byte. */
int pssbam_engine_feed_break(pssbam_engine *e);
/* Several engines dealt alternating runs of ONE stream (one BAM over n GPUs): the blocks submitted to `to`
 * from now on continue the stream where the blocks submitted to `from` so far end.  `from`'s pending blocks
 * are processed; the partial record its run ends in (records cross BGZF blocks in files written by htsjdk)
 * travels to `to` -- device to device through page-locked host memory, no host wait -- and is completed,
 * indexed and tallied there, so the record chain is checked across engines as it is inside one.  The
 * reference has no counterpart (one process, one `samtools view` pipe: pss-bam.c:148-162, 764-783). */
int pssbam_engine_feed_handoff(pssbam_engine *from, pssbam_engine *to);
#define PSSBAM_FEED_BAD_BLOCK 1u   /* a block failed inflate / ISIZE / CRC-32                         */
#define PSSBAM_FEED_RAGGED 2u      /* the per-block record chains did not link up (or a record above 16 MiB):
                                      use the host reader for this file                               */
#define PSSBAM_FEED_BAD_RECORD 4u  /* an alignment record with block_size < 32                        */
#define PSSBAM_FEED_TRUNCATED 8u   /* the stream ended inside an alignment record (as of the last sync) */
int pssbam_engine_feed_status(pssbam_engine *e, uint32_t *flags, double *inflate_ms, uint64_t *inflated_bytes);
/* Optional, before pssbam_engine_submit_bgzf / _submit_device: a few whole alignment records in host
 * memory (e.g. the first ones of the file) from which the tiled kernels' staged record prefix is
 * sized -- otherwise the engine reads the first block back from the device to look at its records. */
int pssbam_engine_hint_records(pssbam_engine *e, const void *records, uint64_t nbytes);
/* Optional: allocates two of the feed's slots (2 x (2 GiB compressed + 4.5 GiB inflated) = ~13 GB) for
 * `device` ahead of time, e.g. from a helper thread while the FASTA loads; the first engine on that device
 * that feeds compressed blocks takes them.  pssbam_feed_release frees what no engine took. */
int pssbam_feed_reserve(int device);
int pssbam_feed_release(int device);

/* Test / tool convenience: host BGZF bytes in, inflated bytes out (out may be NULL), kernels timed
 * with HIP events (*kernel_ms = best of `repeats` runs of inflate + CRC). */
int pssbam_bgzf_inflate_host(int device, const void *bgzf, uint64_t nbytes, void *out, uint64_t out_cap, uint64_t *out_len,
                             uint32_t *n_blocks, uint32_t *first_bad_block, uint32_t *first_bad_status, double *kernel_ms,
                             int check_crc, int repeats);

/* Deflates d_raw[0, raw_bytes) into whole BGZF blocks on the current device, asynchronously on hip_stream.  The stream is
 * cut into payloads of 0xFF00 bytes at fixed offsets (the last one short); the blocks are written back to back to d_bgzf
 * and d_totals = {bytes written, blocks}.  d_raw is 16-byte aligned and readable up to the next multiple of 16 bytes;
 * d_bgzf holds bgzf_cap >= raw_bytes + 31 * blocks bytes (blocks = ceil(raw_bytes / 0xFF00); no block is larger than its
 * stored form, 31 bytes over its payload); d_work is 16-byte aligned scratch of work_bytes >=
 * pssbam_bgzf_deflate_work_bytes(raw_bytes): a 64 KiB slot, a length and an offset per block.  d_raw and d_bgzf may not
 * overlap d_work; d_bgzf may be d_raw (the raw bytes are dead once deflated) when d_raw has the capacity.  raw_bytes == 0
 * writes {0, 0}.  PSSBAM_EINVAL for a buffer too small or misaligned. */
uint64_t pssbam_bgzf_deflate_work_bytes(uint64_t raw_bytes);
int pssbam_bgzf_deflate_device(void *hip_stream, const void *d_raw, uint64_t raw_bytes, void *d_bgzf, uint64_t bgzf_cap,
                               uint64_t *d_totals, void *d_work, uint64_t work_bytes);

/* Test / tool convenience: host bytes in, BGZF blocks out (out may be NULL; PSSBAM_EINVAL when out_cap is below the bytes
 * written), kernels timed with HIP events (*kernel_ms = best of `repeats` runs of deflate + pack). */
int pssbam_bgzf_deflate_host(int device, const void *raw, uint64_t nbytes, void *out, uint64_t out_cap, uint64_t *out_len,
                             uint32_t *n_blocks, double *kernel_ms, int repeats);

/* Host helper: walks the block_size chain of an inflated BAM record stream.  Writes up
 * to max_records offsets (+ the end sentinel), returns the number of whole records
 * found (>= 0) or PSSBAM_EFORMAT; *consumed = bytes covered by those records. */
int64_t pssbam_index_records(const void *bytes, uint64_t nbytes, uint32_t *offsets,
                             uint64_t max_records, uint64_t *consumed);

#ifdef __cplusplus
}
#endif
#endif /* PSSBAM_HIP_H */

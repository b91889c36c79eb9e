/*
 * pss-bam_amd/host/frontend.c -- the loop that replaces
 *     popen("samtools view") ; while (fgets) { line2saml ; process_aln }
 * of the reference (pss-bam.c:760-783, fragkon.c:338-363): inflated BAM record batches go
 * to the GPU engines as they are, one engine per device, batches dealt round-robin
 * ("reads shard by record block"); the per-device counter blocks are summed with one RCCL
 * reduce at the end.
 */
#include "frontend.h"
#include "read_groups.h"

#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <signal.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include "bam_reader.h"
#include "bam_writer.h"
#include "device_feed.h"
#include "sam_reader.h"

int frontend_fast_exit = 0;
frontend_options frontend_opts = {.max_mismatches = -1, .interior = -1, .site_context = PSSBAM_SITE_NONE};

/* -C: the map on one engine (0 when there is none) */
static int send_contig_sets(pssbam_engine *e, const frontend_contig_map *m)
{
    return m ? pssbam_engine_set_contig_sets(e, m->n_labels, m->n_names, (const char *const *)m->names, m->set_of) : 0;
}

static int send_regions(pssbam_engine *e, const pss_regions *r)
{
    return r ? pssbam_engine_set_regions(e, r->n_names, (const char *const *)r->names, r->n, r->name_of, r->starts, r->ends) : 0;
}

/* -O: the writer behind the engine's record sink.  It is opened at the first chunk (the input's header is known by then:
 * out_header is set before any engine is fed) or, when no record is kept, at the end; the sink runs on whichever thread
 * calls the engine -- the helper thread while it feeds, run_tally's after the join -- never on two at once. */
static bam_writer *out_writer = NULL;
static const bam_header *out_header = NULL;
static int out_failed = 0;
static char out_err[700];

/* a diagnosed exit(1) elsewhere in the command (an unreadable FASTA, say) while the file is being written: no <out.bam>.tmp stays */
static volatile int out_tmp_live = 0;
static void out_at_exit(void)
{
    if (!out_tmp_live || !frontend_opts.out_bam) return;
    char tmp[4200];
    if ((size_t)snprintf(tmp, sizeof tmp, "%s.tmp", frontend_opts.out_bam) < sizeof tmp) unlink(tmp);
}

static int out_open(void)
{
    static int registered = 0;
    if (out_writer) return 0;
    if (!registered) registered = atexit(out_at_exit) == 0;
    out_tmp_live = 1;
    out_writer = out_header ? bam_writer_open(frontend_opts.out_bam, out_header, frontend_opts.out_level, 0) : NULL;
    if (!out_writer) {
        snprintf(out_err, sizeof out_err, "-O: %s", out_header ? bam_writer_open_error() : "the input's header is not known");
        out_failed = 1;
        out_tmp_live = 0;
        return -1;
    }
    return 0;
}

static int out_sink(void *ctx, const void *records, uint64_t nbytes, uint64_t n_records)
{
    (void)ctx;
    (void)n_records;
    if (out_failed || out_open()) return 1;
    if (bam_writer_append(out_writer, records, (size_t)nbytes)) {
        snprintf(out_err, sizeof out_err, "-O: %s", bam_writer_error(out_writer));
        out_failed = 1;
        return 1;
    }
    return 0;
}

/* -Z: the same behind the engine's block sink -- the blocks are written as they come */
static int out_block_sink(void *ctx, const void *bgzf, uint64_t nbytes, uint64_t n_blocks, uint64_t raw_bytes, uint64_t n_records)
{
    (void)ctx;
    (void)n_blocks;
    (void)raw_bytes;
    (void)n_records;
    if (out_failed || out_open()) return 1;
    if (bam_writer_append_blocks(out_writer, bgzf, (size_t)nbytes)) {
        snprintf(out_err, sizeof out_err, "-O: %s", bam_writer_error(out_writer));
        out_failed = 1;
        return 1;
    }
    return 0;
}

/* gives up what was written so far (the run failed, or starts over with the host reader) */
static void out_discard(void)
{
    if (out_writer) bam_writer_abort(out_writer);
    out_writer = NULL;
    out_tmp_live = 0;
}

/* Start-up work that overlaps the caller's FASTA load.  The reference is serial by construction -- load the
 * genome, then loop over the alignments (pss-bam.c:751-783) -- but only the TALLY needs reference bases: a helper
 * thread brings the HIP runtime up, creates the engines and runs the whole compressed feed (PCIe, inflate, CRC-32,
 * record index: device_feed.c) while init_genome is still parsing.  run_tally() then posts the Genome; the helper
 * uploads it to every engine at once (pssbam_engine_set_genome_async) and the super-batches inflated ahead of it
 * are tallied.  For inputs the device feed does not take (SAM text, PSSBAM_DEVICE_INFLATE=0) the helper only warms
 * the runtime up and page-locks the host reader's slots, as before. */
static bam_reader *early_rd = NULL;
static char early_path[4096];
static int early_registered = 0, early_light = 0;
static pthread_t warmup_thread;
static int warmup_running = 0;

static struct early_feed {
    int want;                       /* engines + feed on the helper thread */
    pssbam_config cfg;
    char *up, *down, *rg;           /* the strings cfg points at */
    uint64_t fasta_bytes;
    pssbam_engine *eng[64];
    char **rg_ids;                  /* -G: the BAM header's @RG IDs, set on every engine after create */
    int n_rg;
    int n_gpus, engines_ok, engines_done, fed, feed_rc, genome_set, failed;
    device_feed_stats dfs;
    char err[600];
    pthread_mutex_t mu;
    pthread_cond_t cv;
    int posted, abandon;            /* posted: the genome upload is enqueued on every engine (by run_tally's thread) */
    double t0, t_hip, t_engines, t_posted, t_upload_dur, t_genome_set, t_genome_set_dur, t_feed_end;
} EF = {.mu = PTHREAD_MUTEX_INITIALIZER, .cv = PTHREAD_COND_INITIALIZER};

/* device_feed.h feed_gate: 1 = genome and references are on every engine.  The upload itself (page-locking the
 * contigs, 3 GB of copies per GPU) is enqueued by run_tally's thread -- 60 ms of host work the feeding thread does
 * not have: its super-batches keep going out meanwhile; here only the reference table follows (a few KB), after
 * which the engine tallies what it inflated ahead. */
static int early_gate(void *ctx, int block)
{
    (void)ctx;
    pthread_mutex_lock(&EF.mu);
    while (!EF.posted && !EF.abandon && block) pthread_cond_wait(&EF.cv, &EF.mu);
    const int abandon = EF.abandon, posted = EF.posted;
    pthread_mutex_unlock(&EF.mu);
    if (abandon) return -1;
    if (!posted) return 0;
    if (!EF.genome_set) {
        const double t = frontend_now_s();
        const bam_header *h = bam_reader_header(early_rd);
        for (int g = 0; g < EF.n_gpus; g++)
            if (pssbam_engine_set_references(EF.eng[g], h->n_ref, (const char *const *)h->ref_name)) {
                snprintf(EF.err, sizeof EF.err, "GPU engine: %s", pssbam_last_error());
                EF.failed = 1;
                return -1;
            }
        EF.genome_set = 1;
        EF.t_genome_set = frontend_now_s() - EF.t0;
        EF.t_genome_set_dur = frontend_now_s() - t;
    }
    return 1;
}

static void early_engines_done(void)
{
    pthread_mutex_lock(&EF.mu);
    EF.engines_done = 1;
    pthread_cond_broadcast(&EF.cv);
    pthread_mutex_unlock(&EF.mu);
}

static int feed_run(int n_gpus);

static void *pin_main(void *arg)
{
    (void)arg;
    device_feed_prefetch_pin();
    return NULL;
}

static void *reserve_main(void *arg)
{
    (void)pssbam_feed_reserve((int)(intptr_t)arg); /* best effort */
    return NULL;
}

typedef struct {
    pssbam_config cfg;
    int32_t n_ref;
    pssbam_engine **out;
    int rc, started;
    char err[400];
} engine_make_job;

/* -y / -Y: the read score of the run, if any, onto one engine */
static int send_read_score(pssbam_engine *e, const frontend_score *sc)
{
    return sc && pssbam_engine_set_read_score(e, sc->weights, sc->n_dist, sc->n_qual, sc->use_filter, sc->min_score, sc->hist_half, sc->hist_shift);
}

/* -c / -b: the sum of the BAM header's LN values (0: SAM text, whose references show up as they come), set before the engines are made */
static uint64_t coverage_positions_hint;

static void coverage_hint_from(const bam_header *h)
{
    uint64_t sum = 0;
    for (int32_t i = 0; h && i < h->n_ref; i++) sum += h->ref_len[i];
    coverage_positions_hint = sum;
}

/* The run's options (frontend_opts) onto one engine; non-zero: pssbam_last_error() says why.  Two are left to the callers, who
 * need them at a place of their own: -A (before feed_open on the helper's engines) and -G (the header's @RG IDs).  A new
 * option is one line here. */
static int apply_options(pssbam_engine *e)
{
    const frontend_options *o = &frontend_opts;
    return (o->min_base_quality > 0 && pssbam_engine_set_min_base_quality(e, o->min_base_quality)) ||
           (o->length_hist > 0 && pssbam_engine_set_length_histogram(e, o->length_hist)) ||
           ((o->mismatch_hist > 0 || o->max_mismatches >= 0) && pssbam_engine_set_mismatches(e, o->mismatch_hist, o->max_mismatches, o->mismatch_tv)) ||
           (o->interior >= 0 && pssbam_engine_set_interior(e, o->interior)) ||
           (o->composition > 0 && pssbam_engine_set_composition(e, o->composition)) || send_read_score(e, o->read_score) ||
           (o->site_context != PSSBAM_SITE_NONE && pssbam_engine_set_site_context(e, o->site_context)) ||
           (o->end_depth > 0 && pssbam_engine_set_end_condition(e, o->end_depth, o->end_cell5, o->end_cell3)) ||
           (o->gapped_reads && pssbam_engine_set_gapped_reads(e, 1)) || send_regions(e, o->regions) ||
           (o->n_length_edges > 0 && pssbam_engine_set_length_bins(e, o->n_length_edges, o->length_edges)) ||
           send_contig_sets(e, o->contig_sets) || (o->replicates > 0 && pssbam_engine_set_replicates(e, o->replicates)) ||
           (o->out_bam && (o->out_deflate ? pssbam_engine_set_block_sink(e, out_block_sink, NULL) : pssbam_engine_set_record_sink(e, out_sink, NULL))) ||
           (o->out_bam && o->out_mask_mode != PSSBAM_END_MASK_OFF && pssbam_engine_set_end_mask(e, o->out_mask_mode, o->out_mask_n5, o->out_mask_n3)) ||
           (o->duplicates && pssbam_engine_set_duplicates(e, 1, 0)) ||
           ((o->coverage || o->coverage_bedgraph || o->coverage_window) && pssbam_engine_set_coverage(e, 1, coverage_positions_hint)) ||
           (o->sites && pssbam_engine_set_sites(e, o->sites->n_names, (const char *const *)o->sites->names, o->sites->n, o->sites->name_of, o->sites->pos0, o->site_trim));
}

static void *engine_make_main(void *arg)
{
    engine_make_job *j = (engine_make_job *)arg;
    /* (-A before feed_open: the planes are sized from its n_ref before the feed works out what memory it may take) */
    if (pssbam_engine_create(&j->cfg, j->out) || (frontend_opts.per_contig && pssbam_engine_set_per_contig(*j->out, 1)) ||
        pssbam_engine_feed_open(*j->out, j->n_ref, EF.fasta_bytes) || apply_options(*j->out) ||
        (EF.n_rg > 0 && pssbam_engine_set_read_groups(*j->out, EF.n_rg, (const char *const *)EF.rg_ids))) {
        j->rc = 1;
        snprintf(j->err, sizeof j->err, "%s", pssbam_last_error());   /* (the message is this thread's) */
    }
    return NULL;
}

static void early_feed_main(void)
{
    const int n = env_gpu_count(); /* the first HIP call: runtime start-up happens here */
    EF.t_hip = frontend_now_s() - EF.t0;
    const int have = pssbam_device_count();
    if (!getenv("PSSBAM_OVERSUBSCRIBE")) /* the feed's device buffers, beside the engine set-up below (detached: they only allocate; one per GPU) */
        for (int g = 0; g < n && g < (have > 0 ? have : 1); g++) {
            pthread_t th;
            if (pthread_create(&th, NULL, reserve_main, (void *)(intptr_t)g) == 0) pthread_detach(th);
        }
    /* the loader's staging slots (already being filled) are page-locked beside the engine set-up too: 320 MB take ~30 ms,
     * which used to sit between "engines up" and the first block going out */
    pthread_t pin_th;
    const int pin_started = pthread_create(&pin_th, NULL, pin_main, NULL) == 0;
    const bam_header *h = bam_reader_header(early_rd);
    out_header = h;   /* -O (the reader lives until run_tally() is through) */
    coverage_hint_from(h);
    if (frontend_opts.group_by_rg && (EF.n_rg = pss_parse_read_groups(h->text, h->l_text, &EF.rg_ids)) < 0) EF.n_rg = 0;
    /* one engine per GPU, all created at once: a device's first touch (context, queues, code objects) takes ~0.08 s, and
     * eight of them one after the other would cost more than the whole command does on one GPU */
    engine_make_job job[64];
    pthread_t th[64];
    for (int g = 0; g < n; g++) {
        job[g].cfg = EF.cfg;
        job[g].cfg.device = have > 0 ? g % have : g;
        job[g].n_ref = h->n_ref;
        job[g].out = &EF.eng[g];
        job[g].rc = 0;
        job[g].started = g > 0 && pthread_create(&th[g], NULL, engine_make_main, &job[g]) == 0;
    }
    for (int g = 0; g < n; g++)
        if (!job[g].started) (void)engine_make_main(&job[g]);   /* engine 0 here; the others too if a thread could not be had */
    for (int g = 0; g < n; g++)
        if (job[g].started) pthread_join(th[g], NULL);
    for (int g = 0; g < n; g++) {
        if (job[g].rc) {
            snprintf(EF.err, sizeof EF.err, "GPU engine %d: %s", g, job[g].err);
            EF.failed = 1;
            EF.n_gpus = n;   /* (whatever was created is destroyed with the rest: NULL entries are skipped) */
            early_engines_done();
            if (pin_started) pthread_join(pin_th, NULL);
            return;
        }
        EF.n_gpus = g + 1;
    }
    EF.engines_ok = 1;
    EF.t_engines = frontend_now_s() - EF.t0;
    early_engines_done();
    { /* the light reader has inflated the file's first records on the host: the engines size their staged
       * record prefix from them (no read-back from the device later) */
        const uint8_t *r0;
        const uint32_t *o0;
        size_t nb0;
        int slot0 = -1;
        if (bam_reader_next_hold(early_rd, &r0, &o0, &nb0, &slot0) > 0)
            for (int g = 0; g < n; g++) (void)pssbam_engine_hint_records(EF.eng[g], r0, nb0);
        if (slot0 >= 0) bam_reader_release(early_rd, slot0);
    }
    if (pin_started) pthread_join(pin_th, NULL);
    const feed_gate gate = {early_gate, NULL};
    EF.feed_rc = run_device_feed(EF.eng, n, early_path, bam_reader_header_bytes(early_rd), feed_run(n), getenv("PSSBAM_STATS") != NULL, &EF.dfs, &gate);
    EF.fed = 1;
    EF.t_feed_end = frontend_now_s() - EF.t0;
}

static void *warmup_main(void *arg)
{
    (void)arg;
    if (EF.want) {
        early_feed_main();
        return NULL;
    }
    const int n = env_gpu_count(); /* the first HIP call: runtime start-up happens here */
    for (int g = 0; g < n; g++) (void)pssbam_warmup(g); /* failures surface in pssbam_engine_create */
    if (early_rd && early_light && !getenv("PSSBAM_OVERSUBSCRIBE"))
        for (int g = 0; g < n; g++) (void)pssbam_feed_reserve(g); /* the device feed's buffers, while the FASTA loads (best effort) */
    if (early_rd && early_light) device_feed_prefetch_pin(); /* the loader's staging slots (already being filled) */
    if (early_rd && !early_light && !getenv("PSSBAM_NO_PIN")) {
        void *base;
        size_t bytes;
        bam_reader_buffer(early_rd, &base, &bytes);
        early_registered = pssbam_host_register(base, bytes) == 0; /* best effort: pageable works too */
    }
    return NULL;
}

/* Feed geometry for n GPUs: every GPU is dealt runs of `run` consecutive batches (a sorted BAM then
 * keeps each GPU's reference working set local) and up to n * run copies are in flight
 * at once, so the reader ring needs that many slots plus two for its own fill / index stages. */
static int feed_run(int n_gpus)
{
    const char *v = getenv("PSSBAM_RUN_BATCHES");
    int run = v ? atoi(v) : (n_gpus > 1 ? 2 : 1);
    return run < 1 ? 1 : run > 8 ? 8 : run;
}

static int feed_slots(int n_gpus)
{
    if (getenv("PSSBAM_SLOTS")) return 0; /* the reader reads the variable itself */
    return n_gpus > 1 ? n_gpus * feed_run(n_gpus) + 2 : 3;
}

static char *dup_or_null(const char *p) { return p ? strdup(p) : NULL; }

void frontend_warmup_start(const pssbam_config *cfg, const char *aln_path, const char *fasta_path)
{
    EF.t0 = frontend_now_s();
    if (aln_path && strlen(aln_path) < sizeof early_path && file_is_bam(aln_path) == 1) {
        char err[256];
        /* device feed: the reader is only asked for the BAM header (two threads, small batches) */
        early_light = device_feed_enabled() && !(cfg && cfg->kernel == PSSBAM_KERNEL_SIMPLE);
        early_rd = early_light ? bam_reader_open_slots(aln_path, 2, (size_t)8 << 20, 3, err, sizeof err)
                               : bam_reader_open_slots(aln_path, 0, 0, feed_slots(getenv("PSSBAM_NGPU") ? atoi(getenv("PSSBAM_NGPU")) : 1), err, sizeof err);
        /* (a failure is reported by run_tally's own open) */
        if (early_rd) strcpy(early_path, aln_path);
        if (early_rd && early_light) device_feed_prefetch(aln_path); /* its loader threads read the first windows meanwhile */
        if (early_rd && early_light && cfg && !getenv("PSSBAM_NO_EARLY_FEED")) {
            EF.want = 1;
            EF.cfg = *cfg;
            EF.cfg.pss.up_ctx = EF.up = dup_or_null(cfg->pss.up_ctx);
            EF.cfg.pss.down_ctx = EF.down = dup_or_null(cfg->pss.down_ctx);
            EF.cfg.read_group = EF.rg = dup_or_null(cfg->read_group);
            struct stat sb;
            EF.fasta_bytes = fasta_path && stat(fasta_path, &sb) == 0 ? (uint64_t)sb.st_size : 0;
        }
    }
    warmup_running = pthread_create(&warmup_thread, NULL, warmup_main, NULL) == 0;
    if (!warmup_running) EF.want = 0;
}

static int same_str(const char *a, const char *b) { return (!a && !b) || (a && b && strcmp(a, b) == 0); }

static int same_config(const pssbam_config *a, const pssbam_config *b)
{
    return a->tally_mask == b->tally_mask && a->kernel == b->kernel && same_str(a->read_group, b->read_group) &&
           (!(a->tally_mask & PSSBAM_TALLY_PSS) ||
            (a->pss.region_len == b->pss.region_len && a->pss.min_read_len == b->pss.min_read_len && a->pss.max_read_len == b->pss.max_read_len &&
             a->pss.min_mq == b->pss.min_mq && a->pss.merged_only == b->pss.merged_only && same_str(a->pss.up_ctx, b->pss.up_ctx) &&
             same_str(a->pss.down_ctx, b->pss.down_ctx))) &&
           (!(a->tally_mask & PSSBAM_TALLY_KMER) ||
            (a->kmer.klen == b->kmer.klen && a->kmer.min_mq == b->kmer.min_mq && a->kmer.min_read_len == b->kmer.min_read_len &&
             a->kmer.max_read_len == b->kmer.max_read_len && a->kmer.merged_only == b->kmer.merged_only));
}

/* ---- the exit that does not make the caller wait ---------------------------------------------------------------
 * Once the reports are on disk the command has nothing left to say, but the kernel still needs 0.2-0.3 s to take the
 * process apart (five hardware queues, ~30 GB of device buffers and their page tables, pinned staging slots -- measured
 * with tools/probe/exit_probe.hip and tools/feed_scan.py, profiles/r03_exit_teardown_probe.txt): a third of the whole
 * command on the 200 M-read shape.  So the work runs in a CHILD forked at the very top of main(), before any thread
 * or HIP call exists; the process the caller started only waits for one byte -- the exit status, sent when the
 * tables are written -- and returns it at once, while the child is dismantled in the background.  A child that
 * ends without sending it (a diagnosed exit(1), a signal) is waited for and its status / signal relayed.
 * PSSBAM_DETACH_EXIT=0 keeps everything in one process (the default when LD_PRELOAD names a ROCm profiler: it
 * brings the GPU runtime up before main, and a fork behind that is not safe). */
static int detach_fd = -1;

void frontend_detach_start(void)
{
    const char *v = getenv("PSSBAM_DETACH_EXIT"), *pre = getenv("LD_PRELOAD");
    /* (profilers live in LD_PRELOAD and bring the GPU runtime up before main: no fork behind them) */
    const int tooling = pre && (strstr(pre, "rocprof") || strstr(pre, "roctracer") || strstr(pre, "roctx") || strstr(pre, "omnitrace") ||
                                strstr(pre, "rocsys"));
    if (v ? atoi(v) == 0 : tooling) return;
    int fds[2];
    if (pipe(fds) != 0) return;
    fflush(NULL);
    const pid_t pid = fork();
    if (pid < 0) {
        close(fds[0]);
        close(fds[1]);
        return;
    }
    if (pid == 0) { /* the worker: carries on into main() */
        close(fds[0]);
        (void)fcntl(fds[1], F_SETFD, FD_CLOEXEC);
        detach_fd = fds[1];
        return;
    }
    close(fds[1]);
    unsigned char st = 0;
    ssize_t n;
    do n = read(fds[0], &st, 1);
    while (n < 0 && errno == EINTR);
    if (n == 1) _exit(st); /* the worker's tables are on disk and everything it had to print is printed */
    int ws = 0;
    while (waitpid(pid, &ws, 0) < 0 && errno == EINTR) {}
    if (WIFSIGNALED(ws)) {
        signal(WTERMSIG(ws), SIG_DFL);
        kill(getpid(), WTERMSIG(ws));
    }
    _exit(WIFEXITED(ws) ? WEXITSTATUS(ws) : 1);
}

int frontend_detached(void) { return detach_fd >= 0; }

void front_end_exit(int status)
{
    fflush(NULL);
    if (detach_fd >= 0) { /* releases the caller; what follows is only the teardown */
        const unsigned char st = (unsigned char)status;
        if (write(detach_fd, &st, 1) != 1) {}
        close(detach_fd);
        detach_fd = -1;
        /* a caller that reads our output through pipes waits for their END, not only for the process it started:
         * the address space (and with it the GPU context) goes before the kernel closes a dying process's files */
        close(0);
        close(1);
        close(2);
    }
    if (frontend_fast_exit) _exit(status);
    exit(status);
}

void front_end_fail(int status)
{
    fflush(NULL);
    _exit(status); /* (a detached worker sends no status byte: the caller's process waits for it and relays this one) */
}

/* seconds since the process was created (exec + dynamic loading included): /proc/self/stat field 22 is the
 * start time in clock ticks after boot (10 ms resolution); -1 if it cannot be read */
double frontend_process_age_s(void)
{
    FILE *f = fopen("/proc/self/stat", "r");
    if (!f) return -1.0;
    char buf[2048];
    const size_t n = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[n] = 0;
    const char *p = strrchr(buf, ')'); /* (the command name may hold spaces) */
    if (!p) return -1.0;
    unsigned long long start = 0;
    int field = 2;
    for (p++; *p && field < 22; p++)
        if (*p == ' ') field++;
    if (field != 22 || sscanf(p, "%llu", &start) != 1) return -1.0;
    struct timespec ts;
    if (clock_gettime(CLOCK_BOOTTIME, &ts) != 0) return -1.0;
    return ts.tv_sec + ts.tv_nsec * 1e-9 - (double)start / (double)sysconf(_SC_CLK_TCK);
}

double frontend_now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}
#define now_s frontend_now_s

int env_gpu_count(void)
{
    const char *v = getenv("PSSBAM_NGPU");
    int want = v ? atoi(v) : 1, have = pssbam_device_count();
    if (want < 1) want = 1;
    if (have < 1) have = 1; /* engine creation reports the real problem */
    /* PSSBAM_OVERSUBSCRIBE: several engines per device (engine g on device g % devices) -- lets
     * the multi-engine path (batch dealing, counter sum) be exercised on a one-GPU machine */
    if (getenv("PSSBAM_OVERSUBSCRIBE")) return want > 64 ? 64 : want;
    return want > have ? have : want;
}

void run_result_free(run_result *res)
{
    pss_free_read_groups(res->group_ids, res->group_ids ? res->n_planes : 0);
    for (int i = 0; res->cov_names && i < res->cov_n; i++) free(res->cov_names[i]);
    free(res->cov_names);
    free(res->cov_held);
    free(res->cov_lengths);
    free(res->cov_per_contig);
    free(res->cov_run_ref);
    free(res->cov_run_start);
    free(res->cov_run_end);
    free(res->cov_run_depth);
    free(res->win_ref);
    free(res->win_start);
    free(res->win_end);
    free(res->win_acgt);
    free(res->win_gc);
    free(res->win_covered);
    free(res->win_depth_sum);
    for (int i = 0; res->allele_names && i < res->allele_n_names; i++) free(res->allele_names[i]);
    free(res->allele_names);
    free(res->allele_ref);
    free(res->allele_pos);
    free(res->allele_base);
    free(res->allele_counts);
    free(res->plane_fwd);
    free(res->plane_rev);
    free(res->plane_k5);
    free(res->plane_k3);
    free(res->hist_fwd);
    free(res->hist_rev);
    free(res->mism_fwd);
    free(res->mism_rev);
    free(res->comp5);
    free(res->comp3);
    free(res->score_fwd);
    free(res->score_rev);
    free(res->site_fwd);
    free(res->site_rev);
    free(res->end_fwd);
    free(res->end_rev);
    for (int k = 0; k < res->n_contigs && res->contig_names; k++) free(res->contig_names[k]);
    free(res->contig_names);
    free(res->contig_fwd);
    free(res->contig_rev);
    free(res->fwd);
    free(res->rev);
    free(res->k5);
    free(res->k3);
    memset(res, 0, sizeof *res);
}

/* -G: the @RG IDs of the input's header go to every engine (and into *res); a header without any leaves the engines
 * ungrouped.  Returns 0 or -1 after a diagnostic. */
static int send_read_groups(pssbam_engine **eng, int n_gpus, const char *text, size_t len, run_result *res)
{
    if ((res->n_planes = pss_parse_read_groups(text, len, &res->group_ids)) < 0) {
        res->n_planes = 0;
        fprintf(stderr, "Error: out of memory\n");
        return -1;
    }
    for (int g = 0; g < n_gpus && res->n_planes > 0; g++)
        if (pssbam_engine_set_read_groups(eng[g], res->n_planes, (const char *const *)res->group_ids)) {
            fprintf(stderr, "Error: GPU engine %d: %s\n", g, pssbam_last_error());
            return -1;
        }
    return 0;
}

static int cmp_str_ptr(const void *a, const void *b) { return strcmp(*(const char *const *)a, *(const char *const *)b); }

/* -C: a label whose contigs cannot receive a read -- none of them is both a reference of the input (or "*", the
 * RNAME of refID -1) and a contig of the genome -- gets all-zero tables: one warning line each */
static void warn_unreached_sets(const frontend_contig_map *m, const Genome *genome, int32_t n_ref, const char *const *ref_names,
                                const char *aln_path)
{
    const char **refs = (const char **)malloc(((size_t)n_ref + 1) * sizeof *refs);
    char *reached = (char *)calloc((size_t)m->n_labels, 1);
    if (!refs || !reached) {
        free(refs);
        free(reached);
        return;
    }
    for (int32_t i = 0; i < n_ref; i++) refs[i] = ref_names[i];
    qsort(refs, (size_t)n_ref, sizeof *refs, cmp_str_ptr);
    for (int k = 0; k < m->n_names; k++) {
        const char *nm = m->names[k];
        if (reached[m->set_of[k]]) continue;
        const int in_input = strcmp(nm, "*") == 0 || bsearch(&nm, refs, (size_t)n_ref, sizeof *refs, cmp_str_ptr) != NULL;
        /* Genome.seqs is sorted by strcmp of the ids (the find_seq order) */
        size_t lo = 0, hi = genome ? genome->n_seqs : 0;
        int in_genome = 0;
        while (in_input && lo < hi && !in_genome) {
            const size_t mid = (lo + hi) / 2;
            const int c = strcmp(nm, genome->seqs[mid]->id);
            if (c == 0) in_genome = 1;
            else if (c < 0) hi = mid;
            else lo = mid + 1;
        }
        reached[m->set_of[k]] = (char)in_genome;
    }
    for (int s = 0; s < m->n_labels; s++)
        if (!reached[s])
            fprintf(stderr, "Warning: -C: no contig of label %s is both a reference of %s and in the FASTA; its tables are all zero.\n",
                    m->labels[s], aln_path);
    free(refs);
    free(reached);
}

int run_tally(const pssbam_config *cfg, Genome *genome, const char *aln_path, int n_gpus, run_result *res)
{
    pssbam_engine *eng[64] = {0};
    char err[512];
    int rc = -1, registered = 0;
    void *buf_base = NULL;
    size_t buf_bytes = 0;
    const double t0 = now_s();
    double t_mark = t0, t_open = 0, t_engine = 0, t_register = 0, t_read = 0, t_submit = 0, t_finish = 0;
    const int verbose = getenv("PSSBAM_STATS") != NULL;
    memset(res, 0, sizeof *res);
    if (n_gpus < 1) n_gpus = 1;
    if (n_gpus > 64) n_gpus = 64;

    /* BGZF BAM, or SAM text (plain / gzip): what `samtools view FILE` accepts */
    const int is_bam = file_is_bam(aln_path);
    bam_reader *rd = NULL;
    sam_reader *sd = NULL;
    int32_t refs_sent = -1;
    if (is_bam < 0) {
        fprintf(stderr, "Error: Unable to open %s.\n", aln_path);
        return -1;
    }
    device_feed_stats dfs;
    memset(&dfs, 0, sizeof dfs);
    int fed_on_device = 0, adopted = 0, light = 0;
    int device_feed = is_bam && device_feed_enabled() && cfg->kernel != PSSBAM_KERNEL_SIMPLE;
    if (warmup_running) { /* HIP is needed from here on; the helper thread may be feeding already */
        const int mine = EF.want && is_bam && strcmp(early_path, aln_path) == 0 && same_config(cfg, &EF.cfg) && device_feed;
        if (EF.want) {
            int upload_ok = 0;
            if (mine) { /* the engines exist a few dozen ms after the runtime is up: normally long before the FASTA is in */
                pthread_mutex_lock(&EF.mu);
                while (!EF.engines_done) pthread_cond_wait(&EF.cv, &EF.mu);
                pthread_mutex_unlock(&EF.mu);
                upload_ok = EF.engines_ok;
                const double tu = now_s();
                /* every GPU's upload is enqueued before any is waited for: the links run side by side, and the
                 * helper thread keeps feeding compressed blocks to the same engines meanwhile */
                for (int g = 0; g < EF.n_gpus && upload_ok; g++)
                    if (pssbam_engine_set_genome_async(EF.eng[g], genome)) {
                        snprintf(EF.err, sizeof EF.err, "GPU engine %d: %s", g, pssbam_last_error());
                        upload_ok = 0;
                    }
                EF.t_upload_dur = now_s() - tu;
            }
            pthread_mutex_lock(&EF.mu);
            if (mine && upload_ok) EF.posted = 1;
            else EF.abandon = 1;
            EF.t_posted = now_s() - EF.t0;
            pthread_cond_broadcast(&EF.cv);
            pthread_mutex_unlock(&EF.mu);
        }
        pthread_join(warmup_thread, NULL);
        warmup_running = 0;
        if (EF.want && mine && EF.engines_ok && !EF.failed && EF.posted) {
            adopted = 1;
            n_gpus = EF.n_gpus;
            for (int g = 0; g < n_gpus; g++) eng[g] = EF.eng[g];
        } else if (EF.want) { /* not this run's file / options, or the helper could not set up: start over below */
            for (int g = 0; g < EF.n_gpus; g++)
                if (EF.eng[g]) pssbam_engine_destroy(EF.eng[g]);
            if (EF.failed && verbose) fprintf(stderr, "[pssbam] early feed not usable (%s): regular start\n", EF.err);
        }
        EF.want = 0;
    }
    /* BAM: inflate on the GPU (device_feed.c) unless switched off or the cross-check kernel is forced;
     * the host reader then only parses the header -- and takes over if the file's records cross BGZF
     * blocks */
    if (is_bam && early_rd && strcmp(early_path, aln_path) == 0) {
        rd = early_rd;
        early_rd = NULL;
        light = early_light;
        if (early_registered) {
            bam_reader_buffer(rd, &buf_base, &buf_bytes);
            registered = 1;
        }
    } else if (is_bam && device_feed) {
        rd = bam_reader_open_slots(aln_path, 2, (size_t)8 << 20, 3, err, sizeof err);
        light = 1;
    } else if (is_bam) rd = bam_reader_open_slots(aln_path, 0, 0, feed_slots(n_gpus), err, sizeof err);
    else sd = sam_reader_open(aln_path, 0, err, sizeof err);
    if (is_bam && !rd && light) { /* e.g. a header larger than the light reader's batches: the full reader decides */
        light = 0;
        device_feed = 0;
        rd = bam_reader_open_slots(aln_path, 0, 0, feed_slots(n_gpus), err, sizeof err);
    }
    if (rd && light && !device_feed) { /* opened early for the device feed, which is not wanted after all */
        bam_reader_close(rd);
        light = 0;
        rd = bam_reader_open_slots(aln_path, 0, 0, feed_slots(n_gpus), err, sizeof err);
    }
    if (!rd && !sd) {
        fprintf(stderr, "Error: Unable to open %s: %s\n", aln_path, err);
        goto done;
    }
    t_open = now_s() - t_mark; t_mark = now_s();
    if (frontend_opts.out_bam) {
        if (!rd) { fprintf(stderr, "Error: -O needs BAM input.\n"); goto done; }
        if (!adopted) out_discard();   /* (a helper whose engines were not taken over may have written) */
        out_header = bam_reader_header(rd);
    }
    if (adopted) {
        /* the helper created the engines, fed the file and (usually) set the genome when it was posted */
        if (EF.feed_rc || EF.failed) {
            if (EF.err[0]) fprintf(stderr, "Error: %s\n", EF.err);
            goto done;
        }
        if (!EF.genome_set) { /* the feed ended before it looked at the gate (a file it does not take) */
            const bam_header *h = bam_reader_header(rd);
            for (int g = 0; g < n_gpus; g++)
                if (pssbam_engine_set_references(eng[g], h->n_ref, (const char *const *)h->ref_name)) {
                    fprintf(stderr, "Error: GPU engine %d: %s\n", g, pssbam_last_error());
                    goto done;
                }
        }
        refs_sent = bam_reader_header(rd)->n_ref;
        dfs = EF.dfs;
        if (frontend_opts.group_by_rg) { /* the helper set these IDs on its engines */
            res->n_planes = EF.n_rg;
            res->group_ids = EF.rg_ids;
            EF.rg_ids = NULL;
            EF.n_rg = 0;
        }
        if (verbose)
            fprintf(stderr, "[pssbam] early feed (helper thread, seconds after start-up began): HIP runtime up %.3f, engines %.3f, genome upload "
                            "enqueued %.3f (took this thread %.3f), references set + put-off tallies launched %.3f (took %.3f), feed drained %.3f\n",
                    EF.t_hip, EF.t_engines, EF.t_posted, EF.t_upload_dur, EF.t_genome_set, EF.t_genome_set_dur, EF.t_feed_end);
    } else {
        coverage_hint_from(rd ? bam_reader_header(rd) : NULL);
        for (int g = 0; g < n_gpus; g++) {
            pssbam_config c = *cfg;
            const int have = pssbam_device_count();
            c.device = have > 0 ? g % have : g;
            if (pssbam_engine_create(&c, &eng[g]) || (frontend_opts.per_contig && pssbam_engine_set_per_contig(eng[g], 1)) || apply_options(eng[g])) {
                fprintf(stderr, "Error: GPU engine %d: %s\n", g, pssbam_last_error());
                goto done;
            }
        }
        /* every GPU's upload is enqueued before the first one is waited for */
        for (int g = 0; g < n_gpus; g++)
            if (pssbam_engine_set_genome_async(eng[g], genome)) {
                fprintf(stderr, "Error: GPU engine %d: %s\n", g, pssbam_last_error());
                goto done;
            }
        /* -G on BAM input: the header is known now (SAM text: once its header lines have been read, below) */
        if (frontend_opts.group_by_rg && rd && send_read_groups(eng, n_gpus, bam_reader_header(rd)->text, bam_reader_header(rd)->l_text, res))
            goto done;
    }
    int groups_sent = !frontend_opts.group_by_rg || rd != NULL;
    t_engine = now_s() - t_mark; t_mark = now_s();
    if (device_feed && rd && !adopted) {
        const bam_header *h = bam_reader_header(rd);
        for (int g = 0; g < n_gpus; g++)
            if (pssbam_engine_set_references(eng[g], h->n_ref, (const char *const *)h->ref_name)) {
                fprintf(stderr, "Error: GPU engine %d: %s\n", g, pssbam_last_error());
                goto done;
            }
        refs_sent = h->n_ref;
        { /* the light reader has inflated the file's first records on the host: let the engines size their
           * staged record prefix from them (no read-back from the device later) */
            const uint8_t *r0;
            const uint32_t *o0;
            size_t nb0;
            int slot0 = -1;
            if (bam_reader_next_hold(rd, &r0, &o0, &nb0, &slot0) > 0)
                for (int g = 0; g < n_gpus; g++) (void)pssbam_engine_hint_records(eng[g], r0, nb0);
            if (slot0 >= 0) bam_reader_release(rd, slot0);
        }
        if (run_device_feed(eng, n_gpus, aln_path, bam_reader_header_bytes(rd), feed_run(n_gpus), verbose, &dfs, NULL)) goto done;
    }
    if (device_feed && rd) {
        if (dfs.fallback) {
            if (verbose) fprintf(stderr, "[pssbam] device feed not usable for this file: falling back to the host reader\n");
            for (int g = 0; g < n_gpus; g++)
                if (pssbam_engine_reset(eng[g])) { fprintf(stderr, "Error: GPU engine %d: %s\n", g, out_failed ? out_err : pssbam_last_error()); goto done; }
            out_discard();   /* -O: the records come again, from the start */
            out_header = NULL;
            bam_reader_close(rd);
            rd = bam_reader_open_slots(aln_path, 0, 0, feed_slots(n_gpus), err, sizeof err);
            light = 0;
            if (!rd) { fprintf(stderr, "Error: Unable to open %s: %s\n", aln_path, err); goto done; }
            out_header = bam_reader_header(rd);
        } else fed_on_device = 1;
        t_submit = now_s() - t_mark; t_mark = now_s();
    }
    if (rd && !fed_on_device && !registered && !getenv("PSSBAM_NO_PIN")) {
        bam_reader_buffer(rd, &buf_base, &buf_bytes);
        registered = pssbam_host_register(buf_base, buf_bytes) == 0; /* best effort: pageable works too */
    }
    t_register = now_s() - t_mark;

    /* Batches in flight: (reader slot, engine, ticket).  A BAM batch is handed to its engine without
     * waiting for the copy (pssbam_engine_submit_async) and its slot goes back to the reader when
     * the copy has completed -- so the PCIe links of different GPUs carry copies at the same time
     * and one host thread is enough to deal them.  SAM text keeps the blocking submit. */
    struct { int slot, g; uint64_t ticket; double t_issue, t_done; } fifo[64];
    int fifo_head = 0, fifo_len = 0;
    const int run = feed_run(n_gpus);
    const int max_inflight = rd ? (bam_reader_slots(rd) - 2 < 1 ? 1 : bam_reader_slots(rd) - 2 > 62 ? 62 : bam_reader_slots(rd) - 2) : 0;
    double overlap_s = 0.0, win_lo[64], win_hi[64]; /* last copy window seen per engine */
    for (int g = 0; g < 64; g++) win_lo[g] = win_hi[g] = -1.0;
    uint64_t n_batches = 0;
#define RETIRE_OLDEST()                                                                                        \
    do {                                                                                                       \
        const int k = fifo_head;                                                                               \
        if (pssbam_engine_wait_copied(eng[fifo[k].g], fifo[k].ticket)) {                                       \
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());                                   \
            goto done;                                                                                         \
        }                                                                                                      \
        if (fifo[k].t_done < 0) fifo[k].t_done = now_s();                                                      \
        bam_reader_release(rd, fifo[k].slot);                                                                  \
        if (verbose && n_gpus > 1) {                                                                           \
            /* time this copy window shares with the latest window of every other engine */                    \
            for (int o = 0; o < n_gpus; o++) {                                                                 \
                if (o == fifo[k].g || win_hi[o] < 0) continue;                                                 \
                const double lo = fifo[k].t_issue > win_lo[o] ? fifo[k].t_issue : win_lo[o];                   \
                const double hi = fifo[k].t_done < win_hi[o] ? fifo[k].t_done : win_hi[o];                     \
                if (hi > lo) overlap_s += hi - lo;                                                             \
            }                                                                                                  \
            if (n_batches <= 24)                                                                               \
                fprintf(stderr, "[pssbam] copy window: engine %d  %.4f .. %.4f s\n", fifo[k].g, fifo[k].t_issue - t0, \
                        fifo[k].t_done - t0);                                                                  \
            win_lo[fifo[k].g] = fifo[k].t_issue;                                                               \
            win_hi[fifo[k].g] = fifo[k].t_done;                                                                \
        }                                                                                                      \
        fifo_head = (fifo_head + 1) % 64;                                                                      \
        fifo_len--;                                                                                            \
    } while (0)

    for (int turn = 0; !fed_on_device; turn++) {
        const uint8_t *recs;
        const uint32_t *offs;
        size_t nbytes;
        int slot = -1;
        t_mark = now_s();
        int64_t n = rd ? bam_reader_next_hold(rd, &recs, &offs, &nbytes, &slot) : sam_reader_next(sd, &recs, &offs, &nbytes);
        t_read += now_s() - t_mark; t_mark = now_s();
        if (n < 0) {
            fprintf(stderr, "Error: %s: %s\n", aln_path, rd ? bam_reader_error(rd) : sam_reader_error(sd));
            goto done;
        }
        if (!groups_sent) { /* SAM text: its header lines are in once the first batch (or the end) is */
            size_t hl = 0;
            const char *ht = sam_reader_header_text(sd, &hl);
            if (send_read_groups(eng, n_gpus, ht, hl, res)) goto done;
            groups_sent = 1;
        }
        if (n == 0) break;
        n_batches++;
        /* reference names: fixed by the BAM header; for SAM text the table grows as new RNAMEs
         * show up, so it is (re)sent whenever it changed */
        const int32_t n_ref = rd ? bam_reader_header(rd)->n_ref : sam_reader_n_ref(sd);
        if (n_ref != refs_sent) {
            const char *const *names = rd ? (const char *const *)bam_reader_header(rd)->ref_name : sam_reader_ref_names(sd);
            for (int g = 0; g < n_gpus; g++)
                if (pssbam_engine_set_references(eng[g], n_ref, names)) {
                    fprintf(stderr, "Error: GPU engine %d: %s\n", g, pssbam_last_error());
                    goto done;
                }
            refs_sent = n_ref;
        }
        const int g = (turn / run) % n_gpus;
        if (rd) {
            uint64_t ticket = 0;
            const double t_issue = now_s();
            if (pssbam_engine_submit_async(eng[g], recs, nbytes, offs, (uint32_t)n, &ticket)) {
                fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
                goto done;
            }
            const int k = (fifo_head + fifo_len) % 64;
            fifo[k].slot = slot; fifo[k].g = g; fifo[k].ticket = ticket; fifo[k].t_issue = t_issue; fifo[k].t_done = -1.0;
            fifo_len++;
            if (verbose && n_gpus > 1) /* note completions as they are seen (the windows printed with PSSBAM_STATS) */
                for (int i = 0; i < fifo_len; i++) {
                    const int q = (fifo_head + i) % 64;
                    if (fifo[q].t_done < 0 && pssbam_engine_copy_done(eng[fifo[q].g], fifo[q].ticket) == 1) fifo[q].t_done = now_s();
                }
            while (fifo_len > max_inflight) RETIRE_OLDEST();
        } else if (pssbam_engine_submit(eng[g], recs, nbytes, offs, (uint32_t)n)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
        t_submit += now_s() - t_mark;
    }
    while (fifo_len > 0) RETIRE_OLDEST();
#undef RETIRE_OLDEST
    if (verbose && n_gpus > 1 && !fed_on_device)
        fprintf(stderr, "[pssbam] feed: %llu batches in runs of %d over %d engines, up to %d copies in flight; copy windows of "
                        "different engines overlapped for %.3f s\n", (unsigned long long)n_batches, run, n_gpus, max_inflight, overlap_s);
    t_mark = now_s();
    if (refs_sent < 0) { /* no alignment at all: the engines still need a (possibly empty) table to finish */
        const int32_t n_ref = rd ? bam_reader_header(rd)->n_ref : sam_reader_n_ref(sd);
        const char *const *names = rd ? (const char *const *)bam_reader_header(rd)->ref_name : sam_reader_ref_names(sd);
        for (int g = 0; g < n_gpus; g++) (void)pssbam_engine_set_references(eng[g], n_ref, names);
    }
    if (pssbam_reduce_counters(eng, n_gpus, 0)) {
        fprintf(stderr, "Error: counter reduce: %s\n", pssbam_last_error());
        goto done;
    }
    if (cfg->tally_mask & PSSBAM_TALLY_PSS) {
        size_t cells = (size_t)(cfg->pss.region_len + 2) * 16;
        res->fwd = (unsigned long *)calloc(cells, sizeof(unsigned long));
        res->rev = (unsigned long *)calloc(cells, sizeof(unsigned long));
    }
    if (cfg->tally_mask & PSSBAM_TALLY_KMER) {
        size_t bins = (size_t)1 << (2 * cfg->kmer.klen);
        res->k5 = (uint64_t *)calloc(bins, sizeof(uint64_t));
        res->k3 = (uint64_t *)calloc(bins, sizeof(uint64_t));
    }
    if (pssbam_engine_finish(eng[0], res->fwd, res->rev, res->k5, res->k3, res->stats)) {
        fprintf(stderr, "Error: GPU engine: %s\n", out_failed ? out_err : pssbam_last_error());
        goto done;
    }
    if (frontend_opts.duplicates) { /* -d: the one engine's table */
        if (pssbam_engine_finish_duplicates(eng[0], res->dup_totals, res->dup_hist, PSS_DUP_HIST_MAX)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
        res->has_duplicates = 1;
    }
    if (frontend_opts.coverage || frontend_opts.coverage_bedgraph || frontend_opts.coverage_window) { /* -c / -b / -w: the one engine's array */
        const int32_t n_ref = rd ? bam_reader_header(rd)->n_ref : sam_reader_n_ref(sd);
        const char *const *names = rd ? (const char *const *)bam_reader_header(rd)->ref_name : sam_reader_ref_names(sd);
        res->cov_n = n_ref;
        res->cov_names = (char **)calloc((size_t)n_ref + 1, sizeof *res->cov_names);
        res->cov_held = (uint8_t *)calloc((size_t)n_ref + 1, 1);
        res->cov_lengths = (uint64_t *)calloc((size_t)n_ref + 1, sizeof(uint64_t));
        res->cov_per_contig = (uint64_t *)calloc(3 * ((size_t)n_ref + 1), sizeof(uint64_t));
        if (!res->cov_names || !res->cov_held || !res->cov_lengths || !res->cov_per_contig) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        for (int32_t i = 0; i < n_ref; i++) {
            const Seq *sq = find_seq(genome, names[i]);
            res->cov_names[i] = strdup(names[i]);
            res->cov_held[i] = sq != NULL;
            res->cov_lengths[i] = sq ? sq->len : 0;
        }
        if (pssbam_engine_finish_coverage(eng[0], 0, n_ref, res->cov_per_contig, res->cov_hist, PSS_COV_HIST_MAX, &res->cov_n_runs)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
        if (frontend_opts.coverage_bedgraph) {
            const size_t room = (size_t)res->cov_n_runs + 1;
            res->cov_run_ref = (int32_t *)malloc(room * sizeof(int32_t));
            res->cov_run_start = (uint32_t *)malloc(room * sizeof(uint32_t));
            res->cov_run_end = (uint32_t *)malloc(room * sizeof(uint32_t));
            res->cov_run_depth = (uint32_t *)malloc(room * sizeof(uint32_t));
            if (!res->cov_run_ref || !res->cov_run_start || !res->cov_run_end || !res->cov_run_depth) { fprintf(stderr, "Error: out of memory\n"); goto done; }
            if (pssbam_engine_finish_coverage_runs(eng[0], res->cov_n_runs, res->cov_run_ref, res->cov_run_start, res->cov_run_end, res->cov_run_depth,
                                                   &res->cov_n_runs)) {
                fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
                goto done;
            }
        }
        if (frontend_opts.coverage_window) {
            const uint32_t w = frontend_opts.coverage_window;
            if (pssbam_engine_finish_coverage_windows(eng[0], w, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, &res->win_n)) {
                fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
                goto done;
            }
            const size_t room = (size_t)res->win_n + 1;
            res->win_ref = (int32_t *)malloc(room * sizeof(int32_t));
            res->win_start = (uint32_t *)malloc(room * sizeof(uint32_t));
            res->win_end = (uint32_t *)malloc(room * sizeof(uint32_t));
            res->win_acgt = (uint32_t *)malloc(room * sizeof(uint32_t));
            res->win_gc = (uint32_t *)malloc(room * sizeof(uint32_t));
            res->win_covered = (uint32_t *)malloc(room * sizeof(uint32_t));
            res->win_depth_sum = (uint64_t *)malloc(room * sizeof(uint64_t));
            if (!res->win_ref || !res->win_start || !res->win_end || !res->win_acgt || !res->win_gc || !res->win_covered || !res->win_depth_sum) {
                fprintf(stderr, "Error: out of memory\n");
                goto done;
            }
            if (pssbam_engine_finish_coverage_windows(eng[0], w, res->win_n, res->win_ref, res->win_start, res->win_end, res->win_acgt, res->win_gc, res->win_covered,
                                                      res->win_depth_sum, &res->win_n)) {
                fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
                goto done;
            }
        }
        res->has_coverage = 1;
    }
    if (frontend_opts.sites) { /* -a: the one engine's site counters */
        const int32_t n_ref = rd ? bam_reader_header(rd)->n_ref : sam_reader_n_ref(sd);
        const char *const *names = rd ? (const char *const *)bam_reader_header(rd)->ref_name : sam_reader_ref_names(sd);
        if (pssbam_engine_finish_sites(eng[0], 0, NULL, NULL, NULL, NULL, &res->allele_n, NULL)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
        const size_t room = (size_t)res->allele_n + 1;
        res->allele_n_names = n_ref;
        res->allele_names = (char **)calloc((size_t)n_ref + 1, sizeof *res->allele_names);
        res->allele_ref = (int32_t *)malloc(room * sizeof(int32_t));
        res->allele_pos = (uint32_t *)malloc(room * sizeof(uint32_t));
        res->allele_base = (uint8_t *)malloc(room);
        res->allele_counts = (uint32_t *)malloc(room * 10 * sizeof(uint32_t));
        if (!res->allele_names || !res->allele_ref || !res->allele_pos || !res->allele_base || !res->allele_counts) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        for (int32_t i = 0; i < n_ref; i++) res->allele_names[i] = strdup(names[i]);
        if (pssbam_engine_finish_sites(eng[0], res->allele_n, res->allele_ref, res->allele_pos, res->allele_base, res->allele_counts, &res->allele_n,
                                       res->allele_totals)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
        res->has_alleles = 1;
    }
    if (frontend_opts.length_hist > 0 && (cfg->tally_mask & PSSBAM_TALLY_PSS)) { /* -H: summed with the rest of the block */
        res->hist_max = frontend_opts.length_hist;
        res->hist_fwd = (uint64_t *)calloc((size_t)res->hist_max + 2, sizeof(uint64_t));
        res->hist_rev = (uint64_t *)calloc((size_t)res->hist_max + 2, sizeof(uint64_t));
        if (!res->hist_fwd || !res->hist_rev) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        if (pssbam_engine_finish_length_histogram(eng[0], res->hist_fwd, res->hist_rev)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
    }
    if (frontend_opts.mismatch_hist > 0 && cfg->tally_mask == PSSBAM_TALLY_PSS) { /* -N: summed with the rest of the block */
        res->mism_max = frontend_opts.mismatch_hist;
        res->mism_fwd = (uint64_t *)calloc((size_t)res->mism_max + 2, sizeof(uint64_t));
        res->mism_rev = (uint64_t *)calloc((size_t)res->mism_max + 2, sizeof(uint64_t));
        if (!res->mism_fwd || !res->mism_rev) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        if (pssbam_engine_finish_mismatches(eng[0], res->mism_fwd, res->mism_rev)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
    }
    if (frontend_opts.interior >= 0 && cfg->tally_mask == PSSBAM_TALLY_PSS) { /* -W: summed with the rest of the block */
        if (pssbam_engine_finish_interior(eng[0], res->interior, &res->interior_reads)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
        res->has_interior = 1;
    }
    if (frontend_opts.composition > 0 && cfg->tally_mask == PSSBAM_TALLY_PSS) { /* -P: summed with the rest of the block */
        const size_t words = (size_t)frontend_opts.composition * 10;
        res->comp5 = (uint64_t *)calloc(words, sizeof(uint64_t));
        res->comp3 = (uint64_t *)calloc(words, sizeof(uint64_t));
        if (!res->comp5 || !res->comp3) {
            fprintf(stderr, "Error: out of memory\n");
            goto done;
        }
        if (pssbam_engine_finish_composition(eng[0], res->comp5, res->comp3)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
        res->composition_width = frontend_opts.composition;
    }
    if (frontend_opts.read_score && frontend_opts.read_score->hist_half > 0 && cfg->tally_mask == PSSBAM_TALLY_PSS) { /* -Y: summed with the rest of the block */
        res->score_half = frontend_opts.read_score->hist_half;
        res->score_fwd = (uint64_t *)calloc(2 * (size_t)res->score_half, sizeof(uint64_t));
        res->score_rev = (uint64_t *)calloc(2 * (size_t)res->score_half, sizeof(uint64_t));
        if (!res->score_fwd || !res->score_rev) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        if (pssbam_engine_finish_read_score(eng[0], res->score_fwd, res->score_rev)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
    }
    if (frontend_opts.site_context != PSSBAM_SITE_NONE && cfg->tally_mask == PSSBAM_TALLY_PSS) { /* -X: summed with the rest of the block */
        const size_t cells = (size_t)(cfg->pss.region_len + 2) * 16;
        res->site_fwd = (unsigned long *)calloc(cells, sizeof(unsigned long));
        res->site_rev = (unsigned long *)calloc(cells, sizeof(unsigned long));
        if (!res->site_fwd || !res->site_rev) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        if (pssbam_engine_finish_site_context(eng[0], res->site_fwd, res->site_rev)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
    }
    if (frontend_opts.end_depth > 0 && cfg->tally_mask == PSSBAM_TALLY_PSS) { /* -E: summed with the rest of the block */
        const size_t cells = (size_t)(cfg->pss.region_len + 2) * 16;
        res->end_fwd = (unsigned long *)calloc(cells, sizeof(unsigned long));
        res->end_rev = (unsigned long *)calloc(cells, sizeof(unsigned long));
        if (!res->end_fwd || !res->end_rev) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        if (pssbam_engine_finish_end_condition(eng[0], res->end_fwd, res->end_rev, res->end_reads)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            goto done;
        }
    }
    if (frontend_opts.per_contig && cfg->tally_mask == PSSBAM_TALLY_PSS) { /* -A: the planes that hold something (the touched words were summed with the block) */
        const int32_t n_ref = rd ? bam_reader_header(rd)->n_ref : sam_reader_n_ref(sd);
        const char *const *names = rd ? (const char *const *)bam_reader_header(rd)->ref_name : sam_reader_ref_names(sd);
        const size_t cells = (size_t)(cfg->pss.region_len + 2) * 16;
        uint8_t *touched = (uint8_t *)calloc((size_t)n_ref + 1, 1);
        if (!touched) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        if (pssbam_engine_finish_contigs(eng[0], 0, n_ref + 1, NULL, NULL, touched)) {
            fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
            free(touched);
            goto done;
        }
        size_t n_touched = 0;
        for (int32_t k = 0; k <= n_ref; k++) n_touched += touched[k];
        res->contig_names = (char **)calloc(n_touched ? n_touched : 1, sizeof(char *));
        res->contig_fwd = (unsigned long *)calloc(cells * (n_touched ? n_touched : 1), sizeof(unsigned long));
        res->contig_rev = (unsigned long *)calloc(cells * (n_touched ? n_touched : 1), sizeof(unsigned long));
        if (!res->contig_names || !res->contig_fwd || !res->contig_rev) { fprintf(stderr, "Error: out of memory\n"); free(touched); goto done; }
        size_t at = 0;
        for (int32_t k = 0; k <= n_ref;) { /* runs of touched neighbours, one read-back each */
            if (!touched[k]) { k++; continue; }
            int32_t end = k;
            while (end <= n_ref && touched[end]) end++;
            if (pssbam_engine_finish_contigs(eng[0], k, end - k, res->contig_fwd + at * cells, res->contig_rev + at * cells, NULL)) {
                fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
                free(touched);
                goto done;
            }
            for (; k < end; k++) res->contig_names[at++] = strdup(k < n_ref ? names[k] : "*");
        }
        res->n_contigs = (int)n_touched;
        free(touched);
    }
    if (frontend_opts.n_length_edges > 0) res->n_planes = frontend_opts.n_length_edges + 1; /* -G: set with the IDs */
    if (frontend_opts.replicates > 0) res->n_planes = frontend_opts.replicates; /* -J */
    if (frontend_opts.contig_sets) {
        res->n_planes = frontend_opts.contig_sets->n_labels;
        warn_unreached_sets(frontend_opts.contig_sets, genome, rd ? bam_reader_header(rd)->n_ref : sam_reader_n_ref(sd),
                            rd ? (const char *const *)bam_reader_header(rd)->ref_name : sam_reader_ref_names(sd), aln_path);
    }
    if (res->n_planes > 0 && cfg->tally_mask == PSSBAM_TALLY_KMER) {
        const size_t bins = (size_t)1 << (2 * cfg->kmer.klen);
        res->plane_k5 = (uint64_t *)calloc(bins * (size_t)res->n_planes, sizeof(uint64_t));
        res->plane_k3 = (uint64_t *)calloc(bins * (size_t)res->n_planes, sizeof(uint64_t));
        if (!res->plane_k5 || !res->plane_k3) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        for (int k = 0; k < res->n_planes; k++)
            if (pssbam_engine_finish_kmer_groups(eng[0], k, res->plane_k5 + k * bins, res->plane_k3 + k * bins)) {
                fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
                goto done;
            }
    } else if (res->n_planes > 0) {
        const size_t cells = (size_t)(cfg->pss.region_len + 2) * 16;
        res->plane_fwd = (unsigned long *)calloc(cells * (size_t)res->n_planes, sizeof(unsigned long));
        res->plane_rev = (unsigned long *)calloc(cells * (size_t)res->n_planes, sizeof(unsigned long));
        if (!res->plane_fwd || !res->plane_rev) { fprintf(stderr, "Error: out of memory\n"); goto done; }
        for (int k = 0; k < res->n_planes; k++)
            if (pssbam_engine_finish_groups(eng[0], k, res->plane_fwd + k * cells, res->plane_rev + k * cells)) {
                fprintf(stderr, "Error: GPU engine: %s\n", pssbam_last_error());
                goto done;
            }
    }
    t_finish = now_s() - t_mark;
    if (verbose) {
        double h2d = 0, ker = 0;
        uint64_t bytes = 0, launches = 0;
        for (int g = 0; g < n_gpus; g++) {
            double a = 0, c = 0;
            uint64_t b = 0, d = 0;
            if (pssbam_engine_phase_times(eng[g], &a, &b, &c, &d) == 0) { h2d += a; bytes += b; ker += c; launches += d; }
        }
        fprintf(stderr, "[pssbam] device: h2d %.3f kernel %.3f s\n", h2d * 1e-3, ker * 1e-3);
        /* what the GPU(s) spent in kernels, all engines summed (genome encode + 4-bit pack: ~6 ms per GPU, not timed) */
        fprintf(stderr, "[pssbam] gpu busy: inflate+crc+index %.3f tally %.3f s over %d engine(s)\n", fed_on_device ? dfs.inflate_ms * 1e-3 : 0.0, ker * 1e-3, n_gpus);
        fprintf(stderr, "[pssbam] device detail: %.2f GB copied (%.1f GB/s while copying), %llu tally launches\n", bytes * 1e-9,
                h2d > 0 ? bytes * 1e-6 / h2d : 0.0, (unsigned long long)launches);
    }
    if (verbose)
        fprintf(stderr, "[pssbam] phases: open %.3f engine+genome %.3f pin %.3f read(wait) %.3f submit %.3f reduce+finish %.3f s\n",
                t_open, t_engine, t_register, t_read, t_submit, t_finish);
    if (verbose && rd && !fed_on_device) {
        double ph[4];
        bam_reader_phase_seconds(rd, ph);
        fprintf(stderr, "[pssbam] reader thread: scan+carry %.3f inflate %.3f index %.3f wait-for-slot %.3f s\n", ph[0], ph[1], ph[2], ph[3]);
    }
    res->inflate_s = fed_on_device ? dfs.inflate_ms * 1e-3 : rd ? bam_reader_inflate_seconds(rd) : 0.0;
    if (sd) res->stats[PSSBAM_ST_PARSE_SKIP] += sam_reader_lines_skipped(sd), res->stats[PSSBAM_ST_RECORDS] += sam_reader_lines_skipped(sd);
    res->n_gpus = n_gpus;
    if (frontend_opts.out_bam) {   /* -O: every kept record has been delivered (finish syncs); the file takes its name now, the last thing that can fail */
        if (out_failed || out_open()) { fprintf(stderr, "Error: %s\n", out_err); goto done; }
        bam_writer *w = out_writer;
        out_writer = NULL;
        const int bad = bam_writer_close(w, err, sizeof err);
        out_tmp_live = 0;
        if (bad) { fprintf(stderr, "Error: -O: %s\n", err); goto done; }
    }
    rc = 0;
done:
    if (rc && out_failed) fprintf(stderr, "Error: %s\n", out_err);
    if (rc) out_discard();   /* -O: a failed run leaves no file behind */
    t_mark = now_s();
    if (!(frontend_fast_exit && rc == 0)) {
        device_feed_prefetch_cancel(); /* a loader opened ahead of time that no feed took over; the staging slots of one that ran */
        for (int g = 0; g < n_gpus; g++)
            if (eng[g]) pssbam_engine_destroy(eng[g]);
        for (int g = 0; g < n_gpus; g++) (void)pssbam_feed_release(g); /* reserved feed buffers no engine took */
        if (registered) pssbam_host_unregister(buf_base);
        bam_reader_close(rd);
        sam_reader_close(sd);
    }
    if (verbose) fprintf(stderr, "[pssbam] teardown %.3f s\n", now_s() - t_mark);
    res->total_s = now_s() - t0;
    if (rc) run_result_free(res);
    return rc;
}

/*
 * pss-bam_amd/host/bam_writer.c -- see bam_writer.h.
 *
 * Blocks are cut into a batch of raw buffers by the caller's thread (block k of the batch at
 * raw + k * BLOCK_MAX).  A full batch is compressed by the pool -- every thread, the caller's
 * included, claims the next block index until none is left -- and then written front to back.
 * Which thread compressed a block has no influence on its bytes: each block is one raw-deflate
 * stream of its own (deflateReset between blocks), so thread count and timing never show in the file.
 */
#include "bam_writer.h"

#include <errno.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <zlib.h>

#define BLOCK_MAX BAM_WRITER_BLOCK_MAX
#define COMP_MAX 0x10000u     /* a BGZF block is at most 64 KiB: BSIZE is 16 bits */
#define BATCH_BLOCKS 256      /* 16 MiB of records between two rounds of the pool */
#define BGZF_HDR 18u
#define BGZF_FTR 8u

static const uint8_t EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43,
                                      0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static __thread char g_open_err[512];

struct bam_writer {
    FILE *fp;
    char *path, *tmp;
    int level, n_workers;      /* pool threads besides the caller's */
    uint8_t *raw, *comp;       /* BATCH_BLOCKS x BLOCK_MAX, BATCH_BLOCKS x COMP_MAX */
    uint32_t raw_len[BATCH_BLOCKS], comp_len[BATCH_BLOCKS];
    int n_blocks;              /* closed blocks of the batch */
    uint32_t cur_len;          /* bytes in the block being filled (block n_blocks) */
    int failed;
    char err[512];
    /* the pool: a round is `total` blocks; `next` is the next unclaimed one, `finished` counts the done ones */
    pthread_t thr[BAM_WRITER_MAX_THREADS];
    pthread_mutex_t mu;
    pthread_cond_t cv_work, cv_done;
    uint64_t round;
    int next, total, finished, stop, comp_failed;
    z_stream zs;               /* the caller's own stream */
    int zs_ready;
};

static void set_err(bam_writer *w, const char *fmt, ...)
{
    if (w->failed) return;   /* the first failure is the one to report */
    w->failed = 1;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(w->err, sizeof w->err, fmt, ap);
    va_end(ap);
}

static int zs_init(z_stream *zs, int level)
{
    memset(zs, 0, sizeof *zs);
    return deflateInit2(zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) == Z_OK ? 0 : -1;
}

/* one BGZF block: header with the BC extra field, raw deflate, CRC-32 and ISIZE.  Returns its length, 0 on failure. */
static uint32_t compress_block(z_stream *zs, const uint8_t *src, uint32_t len, uint8_t *dst)
{
    if (deflateReset(zs) != Z_OK) return 0;
    zs->next_in = (Bytef *)src;
    zs->avail_in = len;
    zs->next_out = dst + BGZF_HDR;
    zs->avail_out = COMP_MAX - BGZF_HDR - BGZF_FTR;
    if (deflate(zs, Z_FINISH) != Z_STREAM_END) return 0;   /* (cannot happen: deflate expands BLOCK_MAX bytes by less than 64) */
    const uint32_t total = BGZF_HDR + (uint32_t)zs->total_out + BGZF_FTR;
    static const uint8_t head[16] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0};
    memcpy(dst, head, 16);
    dst[16] = (uint8_t)((total - 1u) & 0xffu);
    dst[17] = (uint8_t)((total - 1u) >> 8);
    const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), src, len);
    uint8_t *f = dst + total - BGZF_FTR;
    for (int i = 0; i < 4; i++) {
        f[i] = (uint8_t)(crc >> (8 * i));
        f[4 + i] = (uint8_t)(len >> (8 * i));
    }
    return total;
}

/* claims blocks of the current round until none is left; the mutex is held on entry and on return */
static void work_round(bam_writer *w, z_stream *zs)
{
    while (w->next < w->total) {
        const int k = w->next++;
        pthread_mutex_unlock(&w->mu);
        const uint32_t n = compress_block(zs, w->raw + (size_t)k * BLOCK_MAX, w->raw_len[k], w->comp + (size_t)k * COMP_MAX);
        pthread_mutex_lock(&w->mu);
        w->comp_len[k] = n;
        if (!n) w->comp_failed = 1;
        if (++w->finished == w->total) pthread_cond_broadcast(&w->cv_done);
    }
}

static void *worker(void *arg)
{
    bam_writer *w = (bam_writer *)arg;
    z_stream zs;
    const int ok = zs_init(&zs, w->level) == 0;
    uint64_t seen = 0;
    pthread_mutex_lock(&w->mu);
    for (;;) {
        while (!w->stop && w->round == seen) pthread_cond_wait(&w->cv_work, &w->mu);
        if (w->stop) break;
        seen = w->round;
        if (ok) work_round(w, &zs);   /* (a thread without a stream leaves the blocks to the others) */
    }
    pthread_mutex_unlock(&w->mu);
    if (ok) deflateEnd(&zs);
    return NULL;
}

/* compresses and writes the closed blocks of the batch */
static int flush_batch(bam_writer *w)
{
    if (w->failed) return -1;
    if (!w->n_blocks) return 0;
    pthread_mutex_lock(&w->mu);
    w->next = w->finished = 0;
    w->total = w->n_blocks;
    w->round++;
    if (w->n_workers) pthread_cond_broadcast(&w->cv_work);
    work_round(w, &w->zs);
    while (w->finished < w->total) pthread_cond_wait(&w->cv_done, &w->mu);
    w->total = 0;
    const int bad = w->comp_failed;
    pthread_mutex_unlock(&w->mu);
    if (bad) { set_err(w, "deflate failed"); return -1; }
    for (int k = 0; k < w->n_blocks; k++)
        if (fwrite(w->comp + (size_t)k * COMP_MAX, 1, w->comp_len[k], w->fp) != w->comp_len[k]) {
            set_err(w, "cannot write %s: %s", w->tmp, strerror(errno));
            return -1;
        }
    w->n_blocks = 0;   /* (every caller has closed the block being filled: cur_len is 0, the next block starts at the front) */
    return 0;
}

/* closes the block being filled (an empty one is no block) */
static int close_block(bam_writer *w)
{
    if (!w->cur_len) return 0;
    w->raw_len[w->n_blocks++] = w->cur_len;
    w->cur_len = 0;
    return w->n_blocks == BATCH_BLOCKS - 1 ? flush_batch(w) : 0;   /* (a batch is 255 blocks: the last buffer is never used) */
}

/* bytes into the block being filled, a new block whenever it is full (bgzf_write) */
static int put_bytes(bam_writer *w, const uint8_t *p, size_t n)
{
    while (n) {
        const size_t room = BLOCK_MAX - w->cur_len, take = n < room ? n : room;
        memcpy(w->raw + (size_t)w->n_blocks * BLOCK_MAX + w->cur_len, p, take);
        w->cur_len += (uint32_t)take;
        p += take;
        n -= take;
        if (w->cur_len == BLOCK_MAX && close_block(w)) return -1;
    }
    return 0;
}

static void put32(uint8_t *p, uint32_t v)
{
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

static void destroy(bam_writer *w, int remove_tmp)
{
    if (w->n_workers) {
        pthread_mutex_lock(&w->mu);
        w->stop = 1;
        pthread_cond_broadcast(&w->cv_work);
        pthread_mutex_unlock(&w->mu);
        for (int i = 0; i < w->n_workers; i++) pthread_join(w->thr[i], NULL);
    }
    pthread_mutex_destroy(&w->mu);
    pthread_cond_destroy(&w->cv_work);
    pthread_cond_destroy(&w->cv_done);
    if (w->zs_ready) deflateEnd(&w->zs);
    if (w->fp) fclose(w->fp);
    if (remove_tmp && w->tmp) unlink(w->tmp);
    free(w->raw);
    free(w->comp);
    free(w->path);
    free(w->tmp);
    free(w);
}

const char *bam_writer_open_error(void) { return g_open_err; }

bam_writer *bam_writer_open(const char *path, const bam_header *h, int level, int n_threads)
{
    g_open_err[0] = '\0';
    if (!path || !h) { snprintf(g_open_err, sizeof g_open_err, "null argument"); return NULL; }
    if (level < 0 || level > 9) { snprintf(g_open_err, sizeof g_open_err, "compression level %d outside 0..9", level); return NULL; }
    if (n_threads <= 0) {
        const long n = sysconf(_SC_NPROCESSORS_ONLN);
        n_threads = n > 0 ? (int)n : 1;
    }
    if (n_threads > BAM_WRITER_MAX_THREADS) n_threads = BAM_WRITER_MAX_THREADS;
    bam_writer *w = (bam_writer *)calloc(1, sizeof *w);
    if (!w) { snprintf(g_open_err, sizeof g_open_err, "out of memory"); return NULL; }
    pthread_mutex_init(&w->mu, NULL);
    pthread_cond_init(&w->cv_work, NULL);
    pthread_cond_init(&w->cv_done, NULL);
    w->level = level;
    w->path = strdup(path);
    w->tmp = (char *)malloc(strlen(path) + 5);
    w->raw = (uint8_t *)malloc((size_t)BATCH_BLOCKS * BLOCK_MAX);
    w->comp = (uint8_t *)malloc((size_t)BATCH_BLOCKS * COMP_MAX);
    if (!w->path || !w->tmp || !w->raw || !w->comp || zs_init(&w->zs, level)) {
        snprintf(g_open_err, sizeof g_open_err, "out of memory");
        destroy(w, 0);
        return NULL;
    }
    w->zs_ready = 1;
    sprintf(w->tmp, "%s.tmp", path);
    w->fp = fopen(w->tmp, "wb");
    if (!w->fp) {
        snprintf(g_open_err, sizeof g_open_err, "cannot create %s: %s", w->tmp, strerror(errno));
        destroy(w, 0);
        return NULL;
    }
    for (int i = 0; i < n_threads - 1; i++) {
        if (pthread_create(&w->thr[w->n_workers], NULL, worker, w)) break;   /* (fewer threads: the same file, later) */
        w->n_workers++;
    }
    /* the header, in blocks of its own */
    uint8_t word[8] = {'B', 'A', 'M', 1};
    put32(word + 4, h->l_text);
    int rc = put_bytes(w, word, 8);
    if (!rc && h->l_text) rc = put_bytes(w, (const uint8_t *)h->text, h->l_text);
    put32(word, (uint32_t)h->n_ref);
    if (!rc) rc = put_bytes(w, word, 4);
    for (int32_t i = 0; i < h->n_ref && !rc; i++) {
        const size_t l_name = strlen(h->ref_name[i]) + 1;
        put32(word, (uint32_t)l_name);
        rc = put_bytes(w, word, 4);
        if (!rc) rc = put_bytes(w, (const uint8_t *)h->ref_name[i], l_name);
        put32(word, h->ref_len[i]);
        if (!rc) rc = put_bytes(w, word, 4);
    }
    if (!rc) rc = close_block(w);
    if (rc) {
        snprintf(g_open_err, sizeof g_open_err, "%s", w->err);
        destroy(w, 1);
        return NULL;
    }
    return w;
}

int bam_writer_append(bam_writer *w, const void *records, size_t nbytes)
{
    if (!w) return -1;
    if (w->failed) return -1;
    const uint8_t *p = (const uint8_t *)records;
    size_t o = 0;
    while (o < nbytes) {
        if (nbytes - o < 4) { set_err(w, "record set ends inside a record"); return -1; }
        const size_t len = 4 + (size_t)(p[o] | (uint32_t)p[o + 1] << 8 | (uint32_t)p[o + 2] << 16 | (uint32_t)p[o + 3] << 24);
        if (len > nbytes - o) { set_err(w, "record set ends inside a record"); return -1; }
        /* a record that does not fit what is left of the block starts a new one (bam_write1's bgzf_flush_try) */
        if (w->cur_len + len > BLOCK_MAX && close_block(w)) return -1;
        if (put_bytes(w, p + o, len)) return -1;
        o += len;
    }
    return 0;
}

int bam_writer_append_blocks(bam_writer *w, const void *bgzf, size_t nbytes)
{
    if (!w) return -1;
    if (w->failed) return -1;
    /* the BSIZE chain first: nothing is written unless it covers the buffer exactly */
    const uint8_t *p = (const uint8_t *)bgzf;
    static const uint8_t head[4] = {0x1f, 0x8b, 0x08, 0x04};
    for (size_t o = 0; o < nbytes;) {
        if (nbytes - o < BGZF_HDR + BGZF_FTR) { set_err(w, "block set ends inside a BGZF block"); return -1; }
        const uint8_t *b = p + o;
        if (memcmp(b, head, 4) || b[10] != 6 || b[11] != 0 || b[12] != 'B' || b[13] != 'C' || b[14] != 2 || b[15] != 0) {
            set_err(w, "block set: no BGZF header at byte %zu", o);
            return -1;
        }
        const size_t len = (size_t)(b[16] | (uint32_t)b[17] << 8) + 1;
        if (len < BGZF_HDR + BGZF_FTR) { set_err(w, "block set: BSIZE %zu at byte %zu is below a block's frame", len - 1, o); return -1; }
        if (len > nbytes - o) { set_err(w, "block set ends inside a BGZF block"); return -1; }
        o += len;
    }
    if (close_block(w) || flush_batch(w)) return -1;   /* what the writer holds goes first */
    if (nbytes && fwrite(p, 1, nbytes, w->fp) != nbytes) {
        set_err(w, "cannot write %s: %s", w->tmp, strerror(errno));
        return -1;
    }
    return 0;
}

const char *bam_writer_error(const bam_writer *w) { return w ? w->err : "null writer"; }

int bam_writer_close(bam_writer *w, char *err, size_t errlen)
{
    if (!w) return -1;
    int rc = w->failed ? -1 : 0;
    if (!rc) rc = close_block(w);
    if (!rc) rc = flush_batch(w);
    if (!rc && fwrite(EOF_BLOCK, 1, sizeof EOF_BLOCK, w->fp) != sizeof EOF_BLOCK) {
        set_err(w, "cannot write %s: %s", w->tmp, strerror(errno));
        rc = -1;
    }
    if (!rc) {
        FILE *fp = w->fp;
        w->fp = NULL;
        if (fclose(fp)) { set_err(w, "cannot write %s: %s", w->tmp, strerror(errno)); rc = -1; }
    }
    if (!rc && rename(w->tmp, w->path)) { set_err(w, "cannot rename %s to %s: %s", w->tmp, w->path, strerror(errno)); rc = -1; }
    if (rc && err && errlen) snprintf(err, errlen, "%s", w->err);
    destroy(w, rc != 0);
    return rc;
}

void bam_writer_abort(bam_writer *w)
{
    if (w) destroy(w, 1);
}

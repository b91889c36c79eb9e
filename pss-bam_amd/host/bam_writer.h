/*
 * pss-bam_amd/host/bam_writer.h -- BGZF / BAM output (pss-bam -O).
 *
 * The caller hands over whole raw alignment records (le32 block_size + body, back to back, the
 * bytes the reader and the engine's record sink deliver); the writer cuts them into BGZF blocks
 * the way samtools does, compresses the blocks with a pool of threads and writes them in order.
 * The bytes of the file depend on the input and the level alone: the blocks are cut by the
 * calling thread, one after the other, and only their compression runs in parallel.
 *
 * The file grows as <path>.tmp and takes its name in bam_writer_close(); a writer that failed, or
 * that is given up with bam_writer_abort(), leaves nothing behind.
 */
#ifndef PSSBAM_BAM_WRITER_H
#define PSSBAM_BAM_WRITER_H

#include <stddef.h>
#include <stdint.h>

#include "bam_reader.h"

#define BAM_WRITER_BLOCK_MAX 0xFF00u /* payload bytes of one BGZF block (htslib's BGZF_BLOCK_SIZE) */
#define BAM_WRITER_MAX_THREADS 16

typedef struct bam_writer bam_writer;

/* level 0..9 (0: stored blocks).  n_threads <= 0: one per online CPU; always capped at
 * BAM_WRITER_MAX_THREADS.  The header (magic, l_text, text, n_ref, references) is serialised from h
 * into blocks of its own.  NULL on failure: bam_writer_open_error() says why. */
bam_writer *bam_writer_open(const char *path, const bam_header *h, int level, int n_threads);
const char *bam_writer_open_error(void);
/* Whole records; a block is closed when the next record does not fit, a record larger than a
 * block spans blocks.  0, or -1 (bam_writer_error). */
int bam_writer_append(bam_writer *w, const void *records, size_t nbytes);
/* Whole BGZF blocks made elsewhere (the engine's block sink, pss-bam -O ... -Z), written as they are: what the writer
 * holds (the header's blocks, records of earlier bam_writer_append calls) is closed and written first, so the two calls
 * may be mixed on one writer and the file keeps their order.  The BSIZE chain is walked first: a buffer that is not a whole
 * number of blocks with well-formed BGZF headers fails the call (and the writer) before a byte of it is written.  The
 * payloads are not inflated or checked.  0, or -1 (bam_writer_error). */
int bam_writer_append_blocks(bam_writer *w, const void *bgzf, size_t nbytes);
/* Flushes, writes the EOF block, closes the file and renames it to its path.  0, or -1 after
 * removing the temporary file; the writer is freed either way (read the reason first with
 * bam_writer_error -- or pass err). */
int bam_writer_close(bam_writer *w, char *err, size_t errlen);
/* Gives the file up: closes and removes the temporary file, frees the writer. */
void bam_writer_abort(bam_writer *w);
const char *bam_writer_error(const bam_writer *w);

#endif

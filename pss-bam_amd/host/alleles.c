/* pss-bam_amd/host/alleles.c -- see alleles.h */
#include "alleles.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pssbam_hip.h"

static void say(char *err, size_t cap, const char *fmt, ...)
{
    if (!cap) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, cap, fmt, ap);
    va_end(ap);
}

static int is_blank(char c) { return c == ' ' || c == '\t'; }

/* open addressing over the names seen so far (FNV-1a): slot = index + 1, 0 = empty */
static uint32_t hash_name(const char *s, size_t n)
{
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; i++) h = (h ^ (unsigned char)s[i]) * 16777619u;
    return h;
}

int pss_parse_sites(const char *path, const char *text, size_t len, pss_sites *out, char *err, size_t err_cap)
{
    pss_sites r;
    memset(&r, 0, sizeof r);
    memset(out, 0, sizeof *out);
    if (err_cap) err[0] = '\0';
    size_t cap = 0, cap_names = 0, hsize = 0;
    uint32_t *slots = NULL;
    long line = 0;
    for (size_t a = 0; a < len;) {
        size_t b = a;
        while (b < len && text[b] != '\n') b++;
        const size_t next = b + 1;
        line++;
        if (b > a && text[b - 1] == '\r') b--;
        while (a < b && is_blank(text[a])) a++;
        if (a == b || text[a] == '#') {
            a = next;
            continue;
        }
        size_t f0[2], f1[2];
        int nf = 0;
        for (size_t p = a; p < b && nf < 2;) {
            while (p < b && is_blank(text[p])) p++;
            if (p == b) break;
            f0[nf] = p;
            while (p < b && !is_blank(text[p])) p++;
            f1[nf++] = p;
        }
        if (nf < 2) {
            say(err, err_cap, "-a: %s: line %ld: a site needs two fields (contig, 1-based position)", path, line);
            goto fail;
        }
        uint64_t v = 0;
        int digits = 1;
        for (size_t p = f0[1]; p < f1[1]; p++) {
            if (text[p] < '0' || text[p] > '9') { digits = 0; break; }
            if (v <= 0xFFFFFFFFull) v = v * 10 + (uint64_t)(text[p] - '0');
        }
        if (!digits) {
            say(err, err_cap, "-a: %s: line %ld: the position is not a decimal integer", path, line);
            goto fail;
        }
        if (v == 0 || v > 0x100000000ull) {
            say(err, err_cap, "-a: %s: line %ld: the position is 1-based and at most 2^32", path, line);
            goto fail;
        }
        if (r.n == PSSBAM_MAX_REGIONS) {
            say(err, err_cap, "-a: %s: line %ld: more than %d sites", path, line, PSSBAM_MAX_REGIONS);
            goto fail;
        }
        /* the contig: the one of the line before (a sites file comes contig by contig), known already, or new */
        const size_t nl = f1[0] - f0[0];
        int32_t k = r.n ? r.name_of[r.n - 1] : -1;
        if (k < 0 || strlen(r.names[k]) != nl || memcmp(r.names[k], text + f0[0], nl)) {
            if (2 * ((size_t)r.n_names + 1) > hsize) {
                const size_t hs = hsize ? 2 * hsize : 64;
                uint32_t *s2 = (uint32_t *)calloc(hs, sizeof *s2);
                if (!s2) goto oom;
                for (int32_t j = 0; j < r.n_names; j++) {
                    size_t i = hash_name(r.names[j], strlen(r.names[j])) & (hs - 1);
                    while (s2[i]) i = (i + 1) & (hs - 1);
                    s2[i] = (uint32_t)j + 1;
                }
                free(slots);
                slots = s2;
                hsize = hs;
            }
            size_t i = hash_name(text + f0[0], nl) & (hsize - 1);
            while (slots[i] && !(strlen(r.names[slots[i] - 1]) == nl && !memcmp(r.names[slots[i] - 1], text + f0[0], nl))) i = (i + 1) & (hsize - 1);
            if (!slots[i]) {
                if ((size_t)r.n_names == cap_names) {
                    cap_names = cap_names ? 2 * cap_names : 64;
                    char **t = (char **)realloc(r.names, cap_names * sizeof *t);
                    if (!t) goto oom;
                    r.names = t;
                }
                if (!(r.names[r.n_names] = strndup(text + f0[0], nl))) goto oom;
                slots[i] = (uint32_t)++r.n_names;
            }
            k = (int32_t)slots[i] - 1;
        }
        if ((size_t)r.n == cap) {
            cap = cap ? 2 * cap : 1024;
            int32_t *t0 = (int32_t *)realloc(r.name_of, cap * sizeof *t0);
            if (t0) r.name_of = t0;
            uint32_t *t1 = t0 ? (uint32_t *)realloc(r.pos0, cap * sizeof *t1) : NULL;
            if (t1) r.pos0 = t1;
            if (!t1) goto oom;
        }
        r.name_of[r.n] = k;
        r.pos0[r.n] = (uint32_t)(v - 1);
        r.n++;
        a = next;
    }
    if (!r.n) {
        say(err, err_cap, "-a: %s: the file holds no site (it is empty, or holds only comments)", path);
        goto fail;
    }
    free(slots);
    *out = r;
    return 0;
oom:
    say(err, err_cap, "-a: %s: out of memory reading the sites", path);
fail:
    free(slots);
    pss_free_sites(&r);
    return -1;
}

int pss_read_sites(const char *path, pss_sites *out, char *err, size_t err_cap)
{
    memset(out, 0, sizeof *out);
    FILE *f = fopen(path, "rb");
    char *text = NULL;
    size_t len = 0, cap = 0;
    int read_ok = f != NULL;
    while (read_ok) {
        if (len == cap) {
            char *t = (char *)realloc(text, cap = cap ? 2 * cap : 65536);
            if (!t) { read_ok = 0; break; }
            text = t;
        }
        const size_t got = fread(text + len, 1, cap - len, f);
        len += got;
        if (got == 0) { read_ok = !ferror(f); break; }
    }
    if (f) fclose(f);
    if (!read_ok) {
        free(text);
        say(err, err_cap, "-a: unable to read the sites file %s", path);
        return -1;
    }
    if (len >= 2 && (unsigned char)text[0] == 0x1f && (unsigned char)text[1] == 0x8b) {
        free(text);
        say(err, err_cap, "-a: %s is compressed; only plain text is read", path);
        return -1;
    }
    const int rc = pss_parse_sites(path, text, len, out, err, err_cap);
    free(text);
    return rc;
}

void pss_free_sites(pss_sites *s)
{
    if (!s) return;
    for (int32_t i = 0; i < s->n_names; i++) free(s->names[i]);
    free(s->names);
    free(s->name_of);
    free(s->pos0);
    memset(s, 0, sizeof *s);
}

int pss_write_alleles(const char *fasta_fn, const char *bam_fn, const char *sites_fn, uint32_t trim, const char *out_prefix, int n_names,
                      const char *const *names, uint64_t n_sites, const int32_t *ref, const uint32_t *pos0, const uint8_t *ref_base,
                      const uint32_t *counts, const uint64_t totals[4])
{
    const size_t room = strlen(out_prefix) + 32;
    char *fn = (char *)malloc(room), *tmp = (char *)malloc(room + 8);
    if (!fn || !tmp) {
        fprintf(stderr, "Error: out of memory\n");
        free(fn);
        free(tmp);
        return 1;
    }
    sprintf(fn, "%s.pss.alleles.txt", out_prefix);
    sprintf(tmp, "%s.tmp", fn);
    FILE *fp = fopen(tmp, "w");
    int bad = fp == NULL;
    if (fp) {
        fprintf(fp, "# pss-bam allele counts  fasta %s bam %s sites %s  trim %u\n", fasta_fn, bam_fn, sites_fn, trim);
        fprintf(fp, "# sites_given %llu sites_resolved %llu sites_covered %llu bases_counted %llu\n", (unsigned long long)totals[0],
                (unsigned long long)totals[1], (unsigned long long)totals[2], (unsigned long long)totals[3]);
        fputs("#contig\tpos\tref\tfA\tfC\tfG\tfT\tfO\trA\trC\trG\trT\trO\n", fp);
        for (uint64_t i = 0; i < n_sites && !bad; i++) {
            if (ref[i] < 0 || ref[i] >= n_names) {
                fprintf(stderr, "Error: site %llu names reference %d of %d\n", (unsigned long long)i, (int)ref[i], n_names);
                bad = 1;
                break;
            }
            const uint32_t *c = counts + 10 * i;
            if (fprintf(fp, "%s\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u\n", names[ref[i]], (unsigned long long)pos0[i] + 1ull, (int)ref_base[i], c[0], c[1],
                        c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9]) < 0)
                bad = 1;
        }
        if (fclose(fp)) bad = 1;
        if (!bad && rename(tmp, fn)) bad = 1;
    }
    if (bad) {
        fprintf(stderr, "ERROR: Cannot write to file %s\n.", fn);
        remove(tmp);
    }
    free(fn);
    free(tmp);
    return bad;
}

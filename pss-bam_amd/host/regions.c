/*
 * pss-bam_amd/host/regions.c -- pss-bam -T / fragkon -T: the BED reader.
 */
#include "regions.h"

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

/* decimal digits only, below 2^32: 0 ok, 1 not a number, 2 too large */
static int parse_u32(const char *s, size_t n, uint32_t *out)
{
    if (!n) return 1;
    uint64_t v = 0;
    for (size_t i = 0; i < n; i++) {
        if (s[i] < '0' || s[i] > '9') return 1;
        if (v <= 0xFFFFFFFFull) v = v * 10 + (uint64_t)(s[i] - '0');
    }
    if (v > 0xFFFFFFFFull) return 2;
    *out = (uint32_t)v;
    return 0;
}

/* open addressing over the names seen so far (FNV-1a): slot = index + 1, 0 = empty */
static uint32_t hash_name(const char *s, size_t n)
{
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < n; i++) h = (h ^ (unsigned char)s[i]) * 16777619u;
    return h;
}

int pss_parse_bed(const char *text, size_t len, pss_regions *out, char *err, size_t err_cap)
{
    pss_regions r;
    memset(&r, 0, sizeof r);
    memset(out, 0, sizeof *out);
    if (err_cap) err[0] = '\0';
    size_t cap_iv = 0, cap_names = 0, hsize = 0;
    uint32_t *slots = NULL;
    long line = 0;
    for (size_t a = 0; a < len;) {
        size_t b = a;
        while (b < len && text[b] != '\n') b++;
        const size_t next = b + 1;
        line++;
        if (b > a && text[b - 1] == '\r') b--;
        while (a < b && is_blank(text[a])) a++;
        const size_t ll = b - a;
        if (ll == 0 || text[a] == '#' || (ll >= 5 && !memcmp(text + a, "track", 5)) || (ll >= 7 && !memcmp(text + a, "browser", 7))) {
            a = next;
            continue;
        }
        size_t f0[3], f1[3];
        int nf = 0;
        for (size_t p = a; p < b && nf < 3;) {
            while (p < b && is_blank(text[p])) p++;
            if (p == b) break;
            f0[nf] = p;
            while (p < b && !is_blank(text[p])) p++;
            f1[nf++] = p;
        }
        if (nf < 3) {
            say(err, err_cap, "-T: line %ld: a BED line needs three fields (contig, start, end)", line);
            goto fail;
        }
        uint32_t st = 0, en = 0;
        const int e0 = parse_u32(text + f0[1], f1[1] - f0[1], &st), e1 = parse_u32(text + f0[2], f1[2] - f0[2], &en);
        if (e0 || e1) {
            say(err, err_cap, (e0 ? e0 : e1) == 1 ? "-T: line %ld: the %s coordinate is not a decimal integer"
                                                   : "-T: line %ld: the %s coordinate is 2^32 or above", line, e0 ? "start" : "end");
            goto fail;
        }
        if (st > en) {
            say(err, err_cap, "-T: line %ld: start %u lies behind end %u", line, st, en);
            goto fail;
        }
        if (r.n == PSSBAM_MAX_REGIONS) {
            say(err, err_cap, "-T: line %ld: more than %d intervals", line, PSSBAM_MAX_REGIONS);
            goto fail;
        }
        /* the contig: known already, or new */
        const size_t nl = f1[0] - f0[0];
        if (2 * ((size_t)r.n_names + 1) > hsize) {
            const size_t hs = hsize ? 2 * hsize : 64;
            uint32_t *s2 = (uint32_t *)calloc(hs, sizeof *s2);
            if (!s2) goto oom;
            for (int32_t k = 0; k < r.n_names; k++) {
                size_t i = hash_name(r.names[k], strlen(r.names[k])) & (hs - 1);
                while (s2[i]) i = (i + 1) & (hs - 1);
                s2[i] = (uint32_t)k + 1;
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
        if ((size_t)r.n == cap_iv) {
            cap_iv = cap_iv ? 2 * cap_iv : 1024;
            int32_t *t0 = (int32_t *)realloc(r.name_of, cap_iv * sizeof *t0);
            if (t0) r.name_of = t0;
            uint32_t *t1 = t0 ? (uint32_t *)realloc(r.starts, cap_iv * sizeof *t1) : NULL;
            if (t1) r.starts = t1;
            uint32_t *t2 = t1 ? (uint32_t *)realloc(r.ends, cap_iv * sizeof *t2) : NULL;
            if (t2) r.ends = t2;
            if (!t2) goto oom;
        }
        r.name_of[r.n] = (int32_t)slots[i] - 1;
        r.starts[r.n] = st;
        r.ends[r.n] = en;
        r.n++;
        a = next;
    }
    {
        int64_t usable = 0;
        for (int64_t k = 0; k < r.n; k++) usable += r.starts[k] < r.ends[k];
        if (!usable) {
            say(err, err_cap, "-T: the BED file holds no usable interval (it is empty, or holds only comments and empty intervals)");
            goto fail;
        }
    }
    free(slots);
    *out = r;
    return 0;
oom:
    say(err, err_cap, "-T: out of memory reading the BED file");
fail:
    free(slots);
    pss_free_regions(&r);
    return -1;
}

int pss_read_bed(const char *path, pss_regions *out, char *err, size_t err_cap)
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
        say(err, err_cap, "-T: unable to read the BED file");
        return -1;
    }
    if (len >= 2 && (unsigned char)text[0] == 0x1f && (unsigned char)text[1] == 0x8b) {
        free(text);
        say(err, err_cap, "-T: the BED file is compressed; only plain-text BED is read");
        return -1;
    }
    const int rc = pss_parse_bed(text, len, out, err, err_cap);
    free(text);
    return rc;
}

void pss_free_regions(pss_regions *r)
{
    if (!r) return;
    for (int32_t i = 0; i < r->n_names; i++) free(r->names[i]);
    free(r->names);
    free(r->name_of);
    free(r->starts);
    free(r->ends);
    memset(r, 0, sizeof *r);
}

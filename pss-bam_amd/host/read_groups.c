/*
 * pss-bam_amd/host/read_groups.c -- pss-bam -G: the @RG IDs of a SAM header and the file-name form
 * of an ID.
 */
#include "read_groups.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* value of the line's ID: field (any position after "@RG"), NULL if it has none or an empty one */
static const char *rg_line_id(const char *line, size_t len, size_t *id_len)
{
    size_t i = 3;
    while (i < len) {
        /* i sits on a TAB: the next field runs to the following TAB or the line end */
        size_t f = i + 1, e = f;
        while (e < len && line[e] != '\t') e++;
        if (e - f >= 3 && line[f] == 'I' && line[f + 1] == 'D' && line[f + 2] == ':') {
            *id_len = e - f - 3;
            return *id_len ? line + f + 3 : NULL;
        }
        i = e;
    }
    return NULL;
}

int pss_parse_read_groups(const char *text, size_t len, char ***ids_out)
{
    char **ids = NULL;
    int n = 0, cap = 0;
    *ids_out = NULL;
    if (!text) return 0;
    const size_t tl = strnlen(text, len); /* a BAM header's text may be padded with NULs */
    for (size_t a = 0; a < tl;) {
        size_t b = a;
        while (b < tl && text[b] != '\n') b++;
        size_t e = b;
        if (e > a && text[e - 1] == '\r') e--;
        if (e - a >= 4 && memcmp(text + a, "@RG\t", 4) == 0) {
            size_t il = 0;
            const char *id = rg_line_id(text + a, e - a, &il);
            int dup = 0;
            for (int k = 0; id && k < n && !dup; k++) dup = strlen(ids[k]) == il && memcmp(ids[k], id, il) == 0;
            if (id && !dup) {
                if (n == cap) {
                    cap = cap ? 2 * cap : 16;
                    char **t = (char **)realloc(ids, (size_t)cap * sizeof *ids);
                    if (!t) goto oom;
                    ids = t;
                }
                if (!(ids[n] = strndup(id, il))) goto oom;
                n++;
            }
        }
        a = b + 1;
    }
    *ids_out = ids;
    return n;
oom:
    pss_free_read_groups(ids, n);
    return -1;
}

void pss_free_read_groups(char **ids, int n)
{
    for (int i = 0; i < n; i++) free(ids[i]);
    free(ids);
}

size_t pss_rg_file_tag(const char *id, char *out, size_t cap)
{
    static const char hex[] = "0123456789ABCDEF";
    size_t n = 0;
    for (const unsigned char *p = (const unsigned char *)id; *p; p++) {
        const unsigned c = *p;
        const int plain = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9') || c == '_' || c == '-';
        char enc[3] = {(char)c, 0, 0};
        const size_t k = plain ? 1 : 3;
        if (!plain) enc[0] = '%', enc[1] = hex[c >> 4], enc[2] = hex[c & 15];
        for (size_t j = 0; j < k; j++, n++)
            if (n + 1 < cap) out[n] = enc[j];
    }
    if (cap) out[n < cap ? n : cap - 1] = '\0';
    return n;
}

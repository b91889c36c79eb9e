/*
 * pss-bam_amd/host/contig_sets.c -- pss-bam -C: the contig -> set map file.
 */
#include "contig_sets.h"

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

static uint32_t fnv1a(const char *s)
{
    uint32_t h = 2166136261u;
    for (const unsigned char *p = (const unsigned char *)s; *p; p++) h = (h ^ *p) * 16777619u;
    return h;
}

/* open addressing over strings: slot = index + 1, 0 = empty; grows at half full */
typedef struct {
    uint32_t *slot;
    uint32_t mask;
    int n;
} str_index;

static int index_find(const str_index *x, char **keys, const char *s, uint32_t *at)
{
    uint32_t i = fnv1a(s) & x->mask;
    while (x->slot[i] && strcmp(keys[x->slot[i] - 1], s) != 0) i = (i + 1) & x->mask;
    *at = i;
    return x->slot[i] ? (int)x->slot[i] - 1 : -1;
}

static int index_grow(str_index *x, char **keys)
{
    if (x->slot && (uint32_t)(2 * (x->n + 1)) <= x->mask + 1) return 0;
    const uint32_t size = x->slot ? 2 * (x->mask + 1) : 64;
    uint32_t *slot = (uint32_t *)calloc(size, sizeof *slot);
    if (!slot) return -1;
    str_index y = {slot, size - 1, x->n};
    for (int k = 0; k < x->n; k++) {
        uint32_t at;
        (void)index_find(&y, keys, keys[k], &at);
        slot[at] = (uint32_t)k + 1;
    }
    free(x->slot);
    *x = y;
    return 0;
}

/* appends s[0..len) to *arr (capacity *cap); returns its index or -1 when out of memory */
static int push(char ***arr, int *n, int *cap, const char *s, size_t len)
{
    if (*n == *cap) {
        const int c = *cap ? 2 * *cap : 64;
        char **t = (char **)realloc(*arr, (size_t)c * sizeof *t);
        if (!t) return -1;
        *arr = t;
        *cap = c;
    }
    if (!((*arr)[*n] = strndup(s, len))) return -1;
    return (*n)++;
}

int pss_parse_contig_sets(const char *text, size_t len, char ***names_out, int32_t **set_of_out, char ***labels_out,
                          int *n_labels_out, char *err, size_t err_cap)
{
    char **names = NULL, **labels = NULL;
    int32_t *set_of = NULL;
    int *line_of = NULL;   /* line number of each name's first appearance */
    int n_names = 0, cap_names = 0, n_labels = 0, cap_labels = 0, cap_set = 0;
    str_index by_name = {0}, by_label = {0};
    *names_out = NULL;
    *set_of_out = NULL;
    *labels_out = NULL;
    *n_labels_out = 0;
    if (err_cap) err[0] = '\0';
    if (len && memchr(text, '\0', len)) {
        say(err, err_cap, "-C: the map file holds a NUL byte");
        return -1;
    }
    int line = 0;
    for (size_t a = 0; a < len;) {
        size_t b = a;
        while (b < len && text[b] != '\n') b++;
        const size_t next = b + 1;
        line++;
        if (b > a && text[b - 1] == '\r') b--;
        while (a < b && (text[a] == ' ' || text[a] == '\t')) a++;
        while (b > a && (text[b - 1] == ' ' || text[b - 1] == '\t')) b--;
        if (a == b || text[a] == '#') {
            a = next;
            continue;
        }
        size_t ne = a;
        while (ne < b && text[ne] != ' ' && text[ne] != '\t') ne++;
        size_t ls = ne;
        while (ls < b && (text[ls] == ' ' || text[ls] == '\t')) ls++;
        if (ls == b) ls = a;   /* no label: the name itself */
        char *label = strndup(text + ls, b - ls), *name = strndup(text + a, ne - a);
        if (!label || !name) {
            free(label);
            free(name);
            goto oom;
        }
        uint32_t at;
        int set = labels ? index_find(&by_label, labels, label, &at) : -1;
        if (set < 0) {
            if (n_labels == PSSBAM_MAX_CONTIG_SETS) {
                say(err, err_cap, "-C: more than %d labels (line %d: \"%s\")", PSSBAM_MAX_CONTIG_SETS, line, label);
                free(label);
                free(name);
                goto fail;
            }
            if (index_grow(&by_label, labels) || push(&labels, &n_labels, &cap_labels, label, strlen(label)) < 0) {
                free(label);
                free(name);
                goto oom;
            }
            (void)index_find(&by_label, labels, label, &at);
            by_label.slot[at] = (uint32_t)n_labels;
            by_label.n = n_labels;
            set = n_labels - 1;
        }
        free(label);
        const int k = names ? index_find(&by_name, names, name, &at) : -1;
        if (k >= 0) {
            if (set_of[k] != set) {
                say(err, err_cap, "-C: contig %s is listed under two labels: \"%s\" (line %d) and \"%s\" (line %d)", name,
                    labels[set_of[k]], line_of[k], labels[set], line);
                free(name);
                goto fail;
            }
            free(name);   /* the same name under the same label again: harmless */
            a = next;
            continue;
        }
        if (index_grow(&by_name, names)) {
            free(name);
            goto oom;
        }
        if (n_names == cap_set) {
            cap_set = cap_set ? 2 * cap_set : 64;
            int32_t *s = (int32_t *)realloc(set_of, (size_t)cap_set * sizeof *s);
            int *l = s ? (int *)realloc(line_of, (size_t)cap_set * sizeof *l) : NULL;
            if (s) set_of = s;
            if (l) line_of = l;
            if (!s || !l) {
                free(name);
                goto oom;
            }
        }
        set_of[n_names] = set;
        line_of[n_names] = line;
        const int idx = push(&names, &n_names, &cap_names, name, strlen(name));
        free(name);
        if (idx < 0) goto oom;
        (void)index_find(&by_name, names, names[idx], &at);
        by_name.slot[at] = (uint32_t)idx + 1;
        by_name.n = n_names;
        a = next;
    }
    if (n_labels == 0) {
        say(err, err_cap, "-C: the map file lists no contig (it is empty, or holds only blank and # lines)");
        goto fail;
    }
    free(by_name.slot);
    free(by_label.slot);
    free(line_of);
    *names_out = names;
    *set_of_out = set_of;
    *labels_out = labels;
    *n_labels_out = n_labels;
    return n_names;
oom:
    say(err, err_cap, "-C: out of memory reading the map file");
fail:
    free(by_name.slot);
    free(by_label.slot);
    free(line_of);
    pss_free_contig_sets(names, n_names, set_of, labels, n_labels);
    return -1;
}

void pss_free_contig_sets(char **names, int n_names, int32_t *set_of, char **labels, int n_labels)
{
    for (int i = 0; i < n_names; i++) free(names[i]);
    for (int i = 0; i < n_labels; i++) free(labels[i]);
    free(names);
    free(labels);
    free(set_of);
}

/*
 * pss-bam_amd/host/rescale.c -- the quality rescale (hostcheck -k): the rates file and the P(damage) table built from it.
 */
#include "rescale.h"

#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define COL_AG 1    /* columns of a rates row behind its position: AC AG AT CA CG CT GA GC GT TA TC TG */
#define COL_TC 10
#define MAX_FILE_ROWS (1u << 20)
#define LINE_CAP 4096

typedef struct { double *v; uint32_t n, cap; } column;   /* the two columns of a table's rows, [2 * row + {AG, TC}] */

static int column_push(column *c, double ag, double tc)
{
    if (c->n == c->cap) {
        const uint32_t cap = c->cap ? 2 * c->cap : 64;
        double *v = (double *)realloc(c->v, (size_t)cap * 2 * sizeof *v);
        if (!v) return -1;
        c->v = v;
        c->cap = cap;
    }
    c->v[2 * c->n] = ag;
    c->v[2 * c->n + 1] = tc;
    c->n++;
    return 0;
}

/* 0: a row (pos, ag, tc), 1: a '#' line, 2: a blank line, -1: neither */
static int parse_line(const char *line, long *pos, double *ag, double *tc)
{
    const char *p = line;
    while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
    if (*p == '\0') return 2;
    if (*p == '#') return 1;
    if (*p < '0' || *p > '9') return -1;
    char *end = NULL;
    errno = 0;
    *pos = strtol(p, &end, 10);
    if (errno || end == p || *pos < 0 || *pos >= (long)MAX_FILE_ROWS) return -1;
    p = end;
    for (int k = 0; k < 12; k++) {
        if (*p != ' ' && *p != '\t') return -1;
        errno = 0;
        const double v = strtod(p, &end);
        if (errno || end == p || !(v >= 0.0 && v <= 1.0)) return -1;   /* (a NaN fails both comparisons) */
        if (k == COL_AG) *ag = v;
        if (k == COL_TC) *tc = v;
        p = end;
    }
    while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') p++;
    return *p == '\0' ? 0 : -1;
}

int pss_rescale_table(const char *path, int mode, double baseline, pss_rescale *out, char *err, size_t err_cap)
{
    if (mode != PSS_RESCALE_DS && mode != PSS_RESCALE_SS) {
        snprintf(err, err_cap, "-k: unknown mode %d; the modes are ds and ss", mode);
        return -1;
    }
    if (baseline >= 1.0 || baseline != baseline) {
        snprintf(err, err_cap, "-k: the baseline is a rate in [0, 1), not %g", baseline);
        return -1;
    }
    FILE *fp = fopen(path, "r");
    if (!fp) {
        snprintf(err, err_cap, "-k: unable to read the rates file %s", path);
        return -1;
    }
    column tab[2] = {{NULL, 0, 0}, {NULL, 0, 0}};
    char line[LINE_CAP];
    long line_no = 0, first_rev = -1;
    int section = 0, rc = 0;
    const char *why = NULL;
    while (!why && fgets(line, sizeof line, fp)) {
        line_no++;
        if (!strchr(line, '\n') && !feof(fp)) { why = "the line is too long"; break; }
        long pos = 0;
        double ag = 0.0, tc = 0.0;
        const int kind = parse_line(line, &pos, &ag, &tc);
        if (kind == 2) continue;
        if (kind == 1) {
            if (section < 2 && tab[section].n) section++;   /* a '#' line behind rows closes their table */
            continue;
        }
        if (kind < 0) { why = "not a position and twelve rates in [0, 1]"; break; }
        if (section == 0) {
            if ((uint32_t)pos != tab[0].n) { why = "the forward rows are not 0, 1, 2, ..."; break; }
        } else if (section == 1) {
            if (tab[1].n == 0) first_rev = pos;
            else if (pos != first_rev - (long)tab[1].n) { why = "the reverse rows do not descend to 0"; break; }
        } else { why = "a row behind the two tables"; break; }
        if (column_push(&tab[section], ag, tc)) { why = "out of memory"; break; }
    }
    if (!why && ferror(fp)) {
        snprintf(err, err_cap, "-k: unable to read the rates file %s", path);
        rc = -1;
    }
    fclose(fp);
    if (why) {
        snprintf(err, err_cap, "-k: %s line %ld: %s", path, line_no, why);
        rc = -1;
    }
    if (!rc && tab[1].n && (long)tab[1].n != first_rev + 1) {
        snprintf(err, err_cap, "-k: %s line %ld: the reverse rows do not descend to 0", path, line_no);
        rc = -1;
    }
    if (!rc && tab[0].n == 0 && tab[1].n == 0) {
        snprintf(err, err_cap, "-k: %s holds no rows (the tables of a run with -r 0?)", path);
        rc = -1;
    }
    if (!rc && tab[0].n != tab[1].n) {
        snprintf(err, err_cap, "-k: %s: %u forward and %u reverse rows; the two tables of a run have the same", path, tab[0].n, tab[1].n);
        rc = -1;
    }
    if (!rc) {
        const uint32_t R = tab[0].n, rows = R < PSS_RESCALE_MAX_ROWS ? R : PSS_RESCALE_MAX_ROWS;
        const int col3 = mode == PSS_RESCALE_DS ? 0 : 1;
        memset(out, 0, sizeof *out);
        out->mode = mode;
        out->file_rows = R;
        out->rows = rows;
        for (int end = 0; end < 2; end++) {
            /* forward row i is the file's i-th, reverse row i its (R - 1 - i)-th: the file prints the reverse rows descending */
            double b = baseline;
            if (baseline < 0.0) {
                double sum = 0.0;
                for (uint32_t i = R / 2; i < R; i++) sum += end ? tab[1].v[2 * (R - 1 - i) + col3] : tab[0].v[2 * i + 1];
                b = sum / (double)(R - R / 2);
            }
            out->baseline[end] = b;
            for (uint32_t i = 0; i < rows; i++) {
                const double rate = end ? tab[1].v[2 * (R - 1 - i) + col3] : tab[0].v[2 * i + 1];
                const double d = rate > b && rate > 0.0 ? 1.0 - b / rate : 0.0;
                out->rate[end][i] = rate;
                out->damage[end][i] = d;
                uint8_t *t = out->table + ((size_t)end * rows + i) * PSS_RESCALE_QUALS;
                for (int q = 0; q < PSS_RESCALE_QUALS; q++) {
                    double v = q;
                    if (d != 0.0) {
                        v = floor(-10.0 * log10(1.0 - (1.0 - pow(10.0, -q / 10.0)) * (1.0 - d)) + 0.5);
                        if (!(v >= 0.0)) v = 0.0;
                        if (v > q) v = q;
                    }
                    t[q] = (uint8_t)v;
                }
            }
        }
    }
    free(tab[0].v);
    free(tab[1].v);
    return rc;
}

int pss_parse_rescale(const char *arg, pss_rescale *out, char **path_out, char *err, size_t err_cap)
{
    const char *comma = arg ? strchr(arg, ',') : NULL;
    const size_t len = arg ? (comma ? (size_t)(comma - arg) : strlen(arg)) : 0;
    const int mode = len == 2 && !strncmp(arg, "ds", 2) ? PSS_RESCALE_DS : len == 2 && !strncmp(arg, "ss", 2) ? PSS_RESCALE_SS : 0;
    if (!mode) {
        snprintf(err, err_cap, "-k: unknown mode \"%.*s\"; the modes are ds and ss (-k <mode>,<rates file>[,<baseline>])", (int)(len > 40 ? 40 : len), arg ? arg : "");
        return -1;
    }
    if (!comma || comma[1] == '\0' || comma[1] == ',') {
        snprintf(err, err_cap, "-k %.2s needs the rates file of an earlier run (-k <mode>,<rates file>[,<baseline>])", arg);
        return -1;
    }
    char *path = strdup(comma + 1);
    if (!path) {
        snprintf(err, err_cap, "-k: out of memory");
        return -1;
    }
    double baseline = -1.0;
    char *last = strrchr(path, ',');
    if (last && last[1] != '\0') {
        char *end = NULL;
        const double v = strtod(last + 1, &end);
        if (end != last + 1 && *end == '\0') {   /* (a number: the baseline; anything else is part of the file's name) */
            *last = '\0';
            if (!(v >= 0.0 && v < 1.0)) {
                snprintf(err, err_cap, "-k: the baseline is a rate in [0, 1), not %s", last + 1);
                free(path);
                return -1;
            }
            baseline = v;
        }
    }
    const int rc = pss_rescale_table(path, mode, baseline, out, err, err_cap);
    if (!rc && path_out) *path_out = path;
    else free(path);
    return rc;
}

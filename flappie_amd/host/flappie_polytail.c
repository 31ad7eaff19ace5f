/*  flappie_polytail.c -- the host side of flappie --poly-tail (include/flappie_polytail.h): the options and their ranges, the tags of a record, the summary.
 *  The tail is the GPU's (k_polytail, FFHIP_RUN_POLYTAIL).
 */
#include <errno.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_polytail.h"

void flappie_polytail_defaults(flappie_polytail_opts *o) {
    if (NULL == o) return;
    const flappie_polytail_opts d = { 0, 0, 8, -1, 2, 5, 20000, 20, 0.3f };
    *o = d;
}

static int refuse(char *err, size_t errlen, const char *fmt, const char *a, const char *b) {
    if (err && errlen) snprintf(err, errlen, fmt, a ? a : "", b ? b : "");
    return -1;
}

static int whole(const char *name, const char *value, long lo, long hi, const char *range, long *out, char *err, size_t errlen) {
    char *end = NULL;
    errno = 0;
    const long v = strtol(value, &end, 10);
    if (end == value || *end != '\0' || errno || v < lo || v > hi) return refuse(err, errlen, "--poly-tail-%s must be a whole number %s", name, range);
    *out = v;
    return 0;
}

int flappie_polytail_set(flappie_polytail_opts *o, const char *name, const char *value, char *err, size_t errlen) {
    if (NULL == o || NULL == name || NULL == value) return refuse(err, errlen, "no option%s%s", NULL, NULL);
    long v = 0;
    if (0 == strcmp(name, "base")) {
        const char *at = (value[0] && !value[1]) ? strchr("ACGT", value[0]) : NULL;
        if (NULL == at) return refuse(err, errlen, "--poly-tail-%s must be one of A, C, G, T, not %s", name, value);
        o->base = (int)(at - "ACGT");
        return 0;
    }
    if (0 == strcmp(name, "max-sd")) {
        char *end = NULL;
        errno = 0;
        const float f = strtof(value, &end);
        if (end == value || *end != '\0' || errno || !(f >= 0.0f) || !(f <= 1.0e6f)) return refuse(err, errlen, "--poly-tail-%s must be a number from 0 to 1000000%s", name, NULL);
        o->max_sd = f;
        return 0;
    }
    if (0 == strcmp(name, "window")) { if (whole(name, value, 1, 64, "from 1 to 64", &v, err, errlen)) return -1; o->window = (int)v; return 0; }
    if (0 == strcmp(name, "min-calls")) { if (whole(name, value, 0, 64, "from 0 to the window", &v, err, errlen)) return -1; o->min_calls = (int)v; return 0; }
    if (0 == strcmp(name, "gap")) { if (whole(name, value, 0, 16, "from 0 to 16", &v, err, errlen)) return -1; o->gap = (int)v; return 0; }
    if (0 == strcmp(name, "min-windows")) { if (whole(name, value, 1, 1000000000, "from 1 to 1000000000", &v, err, errlen)) return -1; o->min_windows = (int)v; return 0; }
    if (0 == strcmp(name, "search")) { if (whole(name, value, 1, 1000000000, "of samples from 1 to 1000000000", &v, err, errlen)) return -1; o->search = v; return 0; }
    if (0 == strcmp(name, "min-bases")) { if (whole(name, value, 1, 1000000000, "from 1 to 1000000000", &v, err, errlen)) return -1; o->min_bases = (int)v; return 0; }
    return refuse(err, errlen, "--poly-tail-%s is not an option%s", name, NULL);
}

int flappie_polytail_params(const flappie_polytail_opts *o, int stride, ffhip_polytail_params *out, char *err, size_t errlen) {
    if (NULL == o || NULL == out || stride < 1) return refuse(err, errlen, "no options, or a stride below 1%s%s", NULL, NULL);
    const int min_calls = o->min_calls < 0 ? (o->window + 1) / 2 : o->min_calls;
    if (min_calls > o->window) return refuse(err, errlen, "--poly-tail-min-calls must be a whole number from 0 to the window%s%s", NULL, NULL);
    const long R = o->search / ((long)o->window * stride);
    const ffhip_polytail_params p = { o->base, o->from_end ? 1 : 0, o->window, min_calls, o->gap, o->min_windows, (int32_t)(R < 1 ? 1 : R), o->min_bases, o->max_sd };
    *out = p;
    return 0;
}

long flappie_polytail_bases(const ffhip_polytail *rec) {
    return (NULL != rec && 1 == rec->status) ? lround((double)rec->bases) : -1;
}

char *flappie_polytail_tags(const ffhip_polytail *rec, size_t trim_start) {
    if (NULL == rec) return NULL;
    char *out = malloc(160);
    if (NULL == out) return NULL;
    if (1 != rec->status) { strcpy(out, "pt:i:-1"); return out; }
    const size_t first = trim_start + (size_t)rec->first;
    snprintf(out, 160, "pt:i:%ld\tpa:B:i,%zu,%zu\tpr:f:%.9g", flappie_polytail_bases(rec), first, first + (size_t)rec->count, (double)rec->rate);
    return out;
}

int flappie_polytail_count(flappie_polytail_summary *s, const ffhip_polytail *rec) {
    if (NULL == s || NULL == rec) return -1;
    s->reads++;
    if (3 == rec->status) s->no_rate++;
    if (1 != rec->status) return 0;
    if (s->n == s->cap) {
        const size_t cap = s->cap ? 2 * s->cap : 1024;
        float *p = realloc(s->bases, cap * sizeof(float));
        if (NULL == p) return -1;
        s->bases = p;
        s->cap = cap;
    }
    s->bases[s->n++] = rec->bases;
    s->found++;
    return 0;
}

static int by_value(const void *a, const void *b) {
    const float x = *(const float *)a, y = *(const float *)b;
    return (x > y) - (x < y);
}

double flappie_polytail_median(const flappie_polytail_summary *s) {
    if (NULL == s || 0 == s->n) return NAN;
    float *v = malloc(s->n * sizeof(float));
    if (NULL == v) return NAN;
    memcpy(v, s->bases, s->n * sizeof(float));
    qsort(v, s->n, sizeof(float), by_value);
    const double m = (s->n & 1) ? (double)v[s->n / 2] : ((double)v[s->n / 2 - 1] + (double)v[s->n / 2]) / 2.0;
    free(v);
    return m;
}

void flappie_polytail_summary_print(FILE *fp, const flappie_polytail_summary *s) {
    if (NULL == fp || NULL == s) return;
    fprintf(fp, "polytail\treads\t%llu\npolytail\tfound\t%llu\npolytail\tno_rate\t%llu\npolytail\tmedian\t%.1f\n", s->reads, s->found, s->no_rate, flappie_polytail_median(s));
}

void flappie_polytail_summary_free(flappie_polytail_summary *s) {
    if (NULL == s) return;
    free(s->bases);
    memset(s, 0, sizeof *s);
}

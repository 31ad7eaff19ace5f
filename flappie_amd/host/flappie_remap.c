/*  flappie_remap.c -- the host side of flappie --remap (include/flappie_remap.h): the reader of the sequences, start[] and maxdev of a read's moves, the
 *  line of map.tsv, and that line with the read's place on the reference behind it (flappie --remap-from-map).  The mapping is the GPU's (k_remap, FFHIP_RUN_REMAP).
 */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_remap.h"

void flappie_remap_refs_free(flappie_remap_refs *refs) {
    if (NULL == refs) return;
    for (int k = 0; k < refs->n; k++) { if (refs->name) free(refs->name[k]); if (refs->codes) free(refs->codes[k]); }
    free(refs->name); free(refs->codes); free(refs->len); free(refs->bad); free(refs->order);
    free(refs);
}

static flappie_remap_refs *refuse(flappie_remap_refs *refs, char *err, size_t errlen, const char *why) {
    if (err && errlen) snprintf(err, errlen, "%s", why);
    flappie_remap_refs_free(refs);
    return NULL;
}

static const flappie_remap_refs *sort_refs;
static int by_name(const void *x, const void *y) {
    const int a = *(const int *)x, b = *(const int *)y, c = strcmp(sort_refs->name[a], sort_refs->name[b]);
    return c ? c : (a > b) - (a < b);
}

flappie_remap_refs *flappie_remap_refs_parse(const char *text, const char *alphabet, char *err, size_t errlen) {
    if (NULL == text || NULL == alphabet) return refuse(NULL, err, errlen, "no text");
    flappie_remap_refs *refs = calloc(1, sizeof(*refs));
    if (NULL == refs) return refuse(NULL, err, errlen, "out of memory");
    size_t cap = 0, scap = 0;
    for (const char *p = text; *p; ) {
        const char *eol = p + strcspn(p, "\n");
        const char *a = p, *b = eol;
        while (a < b && isspace((unsigned char)*a)) a++;
        while (b > a && isspace((unsigned char)b[-1])) b--;
        p = *eol ? eol + 1 : eol;
        if (a == b) continue;
        if ('>' == *a) {
            const char *e = a + 1;
            while (e < b && !isspace((unsigned char)*e)) e++;
            if (e == a + 1) return refuse(refs, err, errlen, "a header without a name");
            if ((size_t)refs->n == cap) {
                cap = cap ? 2 * cap : 64;
                char **nm = realloc(refs->name, cap * sizeof(char *));
                if (nm) refs->name = nm;
                uint8_t **cd = realloc(refs->codes, cap * sizeof(uint8_t *));
                if (cd) refs->codes = cd;
                size_t *ln = realloc(refs->len, cap * sizeof(size_t));
                if (ln) refs->len = ln;
                int *bd = realloc(refs->bad, cap * sizeof(int));
                if (bd) refs->bad = bd;
                if (!nm || !cd || !ln || !bd) return refuse(refs, err, errlen, "out of memory");
            }
            refs->codes[refs->n] = NULL; refs->len[refs->n] = 0; refs->bad[refs->n] = 0;
            if (NULL == (refs->name[refs->n] = strndup(a + 1, (size_t)(e - a - 1)))) return refuse(refs, err, errlen, "out of memory");
            refs->n++;
            scap = 0;
            continue;
        }
        if (0 == refs->n) return refuse(refs, err, errlen, "text in front of the first record");
        const int k = refs->n - 1;
        for (const char *c = a; c < b; c++) {
            if (isspace((unsigned char)*c)) continue;
            const char u = (char)toupper((unsigned char)*c);
            const char *at = u ? strchr(alphabet, u) : NULL;
            if (NULL == at) { refs->bad[k] = 1; continue; }
            if (refs->len[k] == scap) {
                scap = scap ? 2 * scap : 256;
                uint8_t *cd = realloc(refs->codes[k], scap);
                if (NULL == cd) return refuse(refs, err, errlen, "out of memory");
                refs->codes[k] = cd;
            }
            refs->codes[k][refs->len[k]++] = (uint8_t)(at - alphabet);
        }
    }
    if (NULL == (refs->order = malloc((refs->n ? refs->n : 1) * sizeof(int)))) return refuse(refs, err, errlen, "out of memory");
    for (int k = 0; k < refs->n; k++) refs->order[k] = k;
    sort_refs = refs;
    qsort(refs->order, refs->n, sizeof(int), by_name);
    return refs;
}

flappie_remap_refs *flappie_remap_refs_read(const char *path, const char *alphabet, char *err, size_t errlen) {
    FILE *fh = path ? fopen(path, "r") : NULL;
    if (NULL == fh) return refuse(NULL, err, errlen, "cannot be read");
    size_t cap = (size_t)1 << 16, got = 0;
    char *text = malloc(cap + 1);
    while (text) {
        got += fread(text + got, 1, cap - got, fh);
        if (got < cap) break;
        char *more = realloc(text, 2 * cap + 1);
        if (NULL == more) { free(text); text = NULL; break; }
        text = more; cap *= 2;
    }
    fclose(fh);
    if (NULL == text) return refuse(NULL, err, errlen, "out of memory");
    text[got] = 0;
    if (strlen(text) != got) { free(text); return refuse(NULL, err, errlen, "holds a NUL byte: not a FASTA file"); }
    flappie_remap_refs *refs = flappie_remap_refs_parse(text, alphabet, err, errlen);
    free(text);
    return refs;
}

static int find_name(const flappie_remap_refs *refs, const char *name, size_t n) {
    int lo = 0, hi = refs->n;                   /* the first record whose name is not below `name[0 .. n)` */
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        const char *m = refs->name[refs->order[mid]];
        int c = strncmp(m, name, n);
        if (0 == c && m[n]) c = 1;
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    if (lo < refs->n) { const char *m = refs->name[refs->order[lo]]; if (0 == strncmp(m, name, n) && 0 == m[n]) return refs->order[lo]; }
    return -1;
}

int flappie_remap_refs_find(const flappie_remap_refs *refs, const char *read_id, const char *filename) {
    if (NULL == refs) return -1;
    int k = -1;
    if (read_id && *read_id) k = find_name(refs, read_id, strlen(read_id));
    if (k < 0 && filename && *filename) {
        const char *base = strrchr(filename, '/');
        base = base ? base + 1 : filename;
        k = find_name(refs, base, strlen(base));
        const char *dot = strrchr(base, '.');
        if (k < 0 && dot && dot > base) k = find_name(refs, base, (size_t)(dot - base));
    }
    return k;
}

int flappie_remap_starts(const uint8_t *rm, size_t nblock, size_t L, size_t *start, size_t *maxdev) {
    if (NULL == rm || 0 == L || 0 == nblock) return -1;
    size_t ones = 0;
    for (size_t b = 0; b < nblock; b++) ones += rm[b] ? 1 : 0;
    if (ones != L - 1) return -1;
    size_t p = 0, dev = 0;
    if (start) start[0] = 0;
    for (size_t b = 0; b < nblock; b++) {
        if (rm[b]) { p++; if (start) start[p] = b + 1; }
        const size_t c = (size_t)(((unsigned long long)(b + 1) * (unsigned long long)(L - 1)) / (unsigned long long)nblock);      /* c(b + 1); c(0) = p_0 = 0 */
        const size_t d = p > c ? p - c : c - p;
        if (d > dev) dev = d;
    }
    if (maxdev) *maxdev = dev;
    return 0;
}

/* the columns of a line of map.tsv, without its end */
static long write_fields(FILE *out, const char *name, int status, size_t nblock, int stride, size_t trim_start, size_t L, int band, const uint8_t *rm, float score) {
    if (1 != status) {
        fprintf(out, "%s\t%d\t%zu\t%d\t%zu\t%zu\t%d\t*\t*\t*", name, status, nblock, stride, trim_start, L, band);
        return 0;
    }
    size_t *start = malloc((L ? L : 1) * sizeof(size_t)), maxdev = 0;
    if (NULL == start || 0 != flappie_remap_starts(rm, nblock, L, start, &maxdev)) { free(start); return -1; }
    fprintf(out, "%s\t%d\t%zu\t%d\t%zu\t%zu\t%d\t%zu\t%.9g\t", name, status, nblock, stride, trim_start, L, band, maxdev, (double)score);
    for (size_t i = 0; i < L; i++) fprintf(out, i ? ",%zu" : "%zu", start[i]);
    free(start);
    return (long)maxdev;
}

long flappie_remap_write_line(FILE *out, const char *name, int status, size_t nblock, int stride, size_t trim_start, size_t L, int band, const uint8_t *rm, float score) {
    const long dev = write_fields(out, name, status, nblock, stride, trim_start, L, band, rm, score);
    if (dev >= 0) fputc('\n', out);
    return dev;
}

long flappie_remap_write_placed_line(FILE *out, const char *name, int status, size_t nblock, int stride, size_t trim_start, size_t L, int band, const uint8_t *rm, float score,
                                     const char *record, char strand, long tstart, long tend) {
    if (NULL == out || NULL == name || NULL == record || ('+' != strand && '-' != strand) || tstart < 0 || tend < tstart) return -1;
    const long dev = write_fields(out, name, status, nblock, stride, trim_start, L, band, rm, score);
    if (dev >= 0) fprintf(out, "\t%s\t%c\t%ld\t%ld\n", record, strand, tstart, tend);
    return dev;
}

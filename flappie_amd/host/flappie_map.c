/*  flappie_map.c -- the host side of flappie --map (include/flappie_map.h): the reference's parser, the turn to forward coordinates, the line of hits.tsv, the
 *  record of --map-records, the summary.  The search is the GPU's (k_map_scan, k_map_finish, FFHIP_RUN_MAP).
 */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_map.h"

void flappie_map_ref_free(flappie_map_ref *ref) {
    if (NULL == ref) return;
    for (int k = 0; k < ref->n; k++) { if (ref->name) free(ref->name[k]); if (ref->seq) free(ref->seq[k]); }
    free(ref->name);
    free(ref->seq);
    free(ref->len);
    free(ref);
}

static flappie_map_ref *refuse(flappie_map_ref *ref, char *err, size_t errlen, const char *fmt, int a, const char *s, size_t at) {
    if (err && errlen) snprintf(err, errlen, fmt, a, s ? s : "", at);
    flappie_map_ref_free(ref);
    return NULL;
}

flappie_map_ref *flappie_map_ref_parse(const char *text, char *err, size_t errlen) {
    if (NULL == text) return refuse(NULL, err, errlen, "no reference text%.0d%s%.0zu", 0, NULL, 0);
    flappie_map_ref *ref = calloc(1, sizeof(*ref));
    if (ref) {
        ref->name = calloc(FLAPPIE_MAP_MAX_RECORDS, sizeof(char *));
        ref->seq = calloc(FLAPPIE_MAP_MAX_RECORDS, sizeof(char *));
        ref->len = calloc(FLAPPIE_MAP_MAX_RECORDS, sizeof(size_t));
    }
    if (NULL == ref || NULL == ref->name || NULL == ref->seq || NULL == ref->len) return refuse(ref, err, errlen, "out of memory%.0d%s%.0zu", 0, NULL, 0);
    size_t total = 0, cap = 0;            /* bases of all records; room of the record being read */
    for (const char *p = text; *p; ) {
        const char *eol = p + strcspn(p, "\n");
        const char *a = p, *b = eol;
        while (a < b && isspace((unsigned char)*a)) a++;
        while (b > a && isspace((unsigned char)b[-1])) b--;
        p = *eol ? eol + 1 : eol;
        if (a == b) continue;
        const int k = ref->n - 1;
        if ('>' == *a) {
            if (k >= 0 && 0 == ref->len[k]) return refuse(ref, err, errlen, "record %d (%s) has no sequence%.0zu", ref->n, ref->name[k], 0);
            if (ref->n == FLAPPIE_MAP_MAX_RECORDS) return refuse(ref, err, errlen, "more than %d records%s%.0zu", FLAPPIE_MAP_MAX_RECORDS, NULL, 0);
            const char *e = a + 1;
            while (e < b && !isspace((unsigned char)*e)) e++;
            if (e == a + 1) return refuse(ref, err, errlen, "record %d has no name%s%.0zu", ref->n + 1, NULL, 0);
            char *name = strndup(a + 1, (size_t)(e - a - 1));
            if (NULL == name) return refuse(ref, err, errlen, "out of memory%.0d%s%.0zu", 0, NULL, 0);
            ref->name[ref->n++] = name;
            cap = 0;
            for (int j = 0; j + 1 < ref->n; j++)
                if (0 == strcmp(ref->name[j], name)) return refuse(ref, err, errlen, "record %d: the name %s occurs twice%.0zu", ref->n, name, 0);
            continue;
        }
        if (k < 0) return refuse(ref, err, errlen, "text in front of the first record%.0d%s%.0zu", 0, NULL, 0);
        const size_t more = (size_t)(b - a);
        if (ref->len[k] + more + 1 > cap) {
            cap = 2 * (ref->len[k] + more) + 64;
            char *grown = realloc(ref->seq[k], cap);
            if (NULL == grown) return refuse(ref, err, errlen, "out of memory%.0d%s%.0zu", 0, NULL, 0);
            ref->seq[k] = grown;
        }
        for (const char *c = a; c < b; c++) {
            if (isspace((unsigned char)*c)) continue;
            const char u = (char)toupper((unsigned char)*c);
            if (NULL == strchr("ACGT", u) || 0 == u)
                return refuse(ref, err, errlen, "record %d (%s): position %zu is not one of ACGT (N and IUPAC letters are not guessed)", ref->n, ref->name[k], ref->len[k]);
            if (total == FFHIP_MAP_MAX_TOTAL) return refuse(ref, err, errlen, "record %d (%s): position %zu: more than 1048576 bases in all", ref->n, ref->name[k], ref->len[k]);
            ref->seq[k][ref->len[k]++] = u;
            total++;
        }
        ref->seq[k][ref->len[k]] = 0;
    }
    if (0 == ref->n) return refuse(ref, err, errlen, "the reference is empty%.0d%s%.0zu", 0, NULL, 0);
    if (0 == ref->len[ref->n - 1]) return refuse(ref, err, errlen, "record %d (%s) has no sequence%.0zu", ref->n, ref->name[ref->n - 1], 0);
    return ref;
}

flappie_map_ref *flappie_map_ref_read(const char *path, char *err, size_t errlen) {
    FILE *fh = path ? fopen(path, "r") : NULL;
    if (NULL == fh) return refuse(NULL, err, errlen, "cannot be read%.0d%s%.0zu", 0, NULL, 0);
    /* (a reference that passes holds at most 2^20 bases and 1024 names: a file beyond 4 MiB is refused by size) */
    const size_t cap = (size_t)4 << 20;
    char *text = malloc(cap + 1);
    if (NULL == text) { fclose(fh); return refuse(NULL, err, errlen, "out of memory%.0d%s%.0zu", 0, NULL, 0); }
    const size_t got = fread(text, 1, cap + 1, fh);
    fclose(fh);
    if (got > cap) { free(text); return refuse(NULL, err, errlen, "larger than 4 MiB: more than 1048576 bases in all%.0d%s%.0zu", 0, NULL, 0); }
    text[got] = 0;
    if (strlen(text) != got) { free(text); return refuse(NULL, err, errlen, "holds a NUL byte: not a FASTA file%.0d%s%.0zu", 0, NULL, 0); }
    flappie_map_ref *ref = flappie_map_ref_parse(text, err, errlen);
    free(text);
    return ref;
}

int flappie_map_forward(const flappie_map_ref *ref, int q, long start, long end, int *record, char *strand, long *fstart, long *fend) {
    if (NULL == ref || q < 0 || (q >> 1) >= ref->n) return -1;
    const long m = (long)ref->len[q >> 1];
    if (start < 0 || end < start || end > m) return -1;
    if (record) *record = q >> 1;
    if (strand) *strand = (q & 1) ? '-' : '+';
    if (fstart) *fstart = (q & 1) ? m - end : start;
    if (fend) *fend = (q & 1) ? m - start : end;
    return 0;
}

int flappie_map_write_line(FILE *out, const char *name, const ffhip_map_call *rec, const flappie_map_ref *ref) {
    if (NULL == out || NULL == name || NULL == rec || NULL == ref || rec->status < 0 || rec->status > 3) return -1;
    int k[3] = { 0, 0, 0 };
    char o[3] = { '*', '*', '*' };
    long a[3] = { 0, 0, 0 }, b[3] = { 0, 0, 0 };
    if (1 == rec->status && 0 != flappie_map_forward(ref, rec->q, rec->tstart, rec->tend, &k[0], &o[0], &a[0], &b[0])) return -1;
    if (rec->status >= 2)
        for (int i = 0; i < 2; i++)
            if (0 != flappie_map_forward(ref, rec->anchor[i].q, rec->anchor[i].start, rec->anchor[i].end, &k[1 + i], &o[1 + i], &a[1 + i], &b[1 + i])) return -1;
    fprintf(out, "%s\t%d\t%d\t%d\t", name, (int)rec->status, (int)rec->n, (int)rec->nanchor);
    if (1 == rec->status) fprintf(out, "%s\t%c\t%ld\t%ld\t%zu", ref->name[k[0]], o[0], a[0], b[0], ref->len[k[0]]);
    else fputs("*\t*\t*\t*\t*", out);
    fprintf(out, "\t%d\t%d\t%d\t%d", (int)rec->anchor[0].dist, (int)rec->anchor[0].second, (int)rec->anchor[1].dist, (int)rec->anchor[1].second);
    if (rec->status >= 2) for (int i = 1; i < 3; i++) fprintf(out, "\t%s\t%c\t%ld\t%ld", ref->name[k[i]], o[i], a[i], b[i]);
    fputc('\n', out);
    return 0;
}

int flappie_map_write_record(FILE *out, const char *name, const ffhip_map_call *rec, const flappie_map_ref *ref) {
    if (NULL == out || NULL == name || NULL == rec || NULL == ref) return -1;
    if (1 != rec->status) return 0;
    int k = 0;
    char o = '+';
    long a = 0, b = 0;
    if (0 != flappie_map_forward(ref, rec->q, rec->tstart, rec->tend, &k, &o, &a, &b)) return -1;
    fprintf(out, ">%s\n", name);
    const char *s = ref->seq[k];
    if ('+' == o) fwrite(s + a, 1, (size_t)(b - a), out);
    else for (long i = b - 1; i >= a; i--) fputc("TGCA"[strchr("ACGT", s[i]) - "ACGT"], out);      /* (the parser let ACGT through only) */
    fputc('\n', out);
    return 1;
}

void flappie_map_summary_add(flappie_map_summary *sum, const ffhip_map_call *rec, int window) {
    if (NULL == sum || NULL == rec) return;
    sum->reads++;
    if (1 == rec->status) {
        const long W = window > 0 ? window : FLAPPIE_MAP_WINDOW_DEFAULT, L = rec->n < W ? rec->n : W;
        sum->mapped++;
        for (int i = 0; i < rec->nanchor && i < 2; i++) { sum->dist += (unsigned long long)rec->anchor[i].dist; sum->bases += (unsigned long long)L; }
    } else if (2 == rec->status) sum->unmapped++;
    else if (3 == rec->status) sum->discordant++;
}

void flappie_map_summary_print(FILE *out, const flappie_map_summary *sum) {
    if (NULL == out || NULL == sum) return;
    fprintf(out, "map\treads\t%llu\nmap\tmapped\t%llu\nmap\tunmapped\t%llu\nmap\tdiscordant\t%llu\nmap\tanchor_dist\t%llu\nmap\tanchor_bases\t%llu\nmap\tpooled_error\t%.6f\n",
            sum->reads, sum->mapped, sum->unmapped, sum->discordant, sum->dist, sum->bases, sum->bases ? (double)sum->dist / (double)sum->bases : 0.0);
}

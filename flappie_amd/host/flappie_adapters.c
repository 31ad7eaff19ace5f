/*  flappie_adapters.c -- the host side of flappie --adapters (include/flappie_adapters.h): the kit's parser, the tags of a record, the trim, the split.
 *  The search is the GPU's (k_adapters, FFHIP_RUN_ADAPTERS).
 */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_adapters.h"

void flappie_adapter_kit_free(flappie_adapter_kit *kit) {
    if (NULL == kit) return;
    for (int k = 0; k < kit->n; k++) { if (kit->name) free(kit->name[k]); if (kit->seq) free(kit->seq[k]); }
    free(kit->name);
    free(kit->seq);
    free(kit);
}

static flappie_adapter_kit *refuse(flappie_adapter_kit *kit, char *err, size_t errlen, const char *fmt, int a, const char *s) {
    if (err && errlen) snprintf(err, errlen, fmt, a, s ? s : "");
    flappie_adapter_kit_free(kit);
    return NULL;
}

flappie_adapter_kit *flappie_adapter_kit_parse(const char *text, char *err, size_t errlen) {
    if (NULL == text) return refuse(NULL, err, errlen, "no kit text%.0d%s", 0, NULL);
    flappie_adapter_kit *kit = calloc(1, sizeof(*kit));
    if (kit) { kit->name = calloc(FLAPPIE_ADAPTER_MAX_KIT, sizeof(char *)); kit->seq = calloc(FLAPPIE_ADAPTER_MAX_KIT, sizeof(char *)); }
    if (NULL == kit || NULL == kit->name || NULL == kit->seq) return refuse(kit, err, errlen, "out of memory%.0d%s", 0, NULL);
    size_t len = 0;                       /* bases of the record being read */
    for (const char *p = text; *p; ) {
        const char *eol = p + strcspn(p, "\n");
        const char *a = p, *b = eol;
        while (a < b && isspace((unsigned char)*a)) a++;
        while (b > a && isspace((unsigned char)b[-1])) b--;
        p = *eol ? eol + 1 : eol;
        if (a == b) continue;
        if ('>' == *a) {
            if (kit->n > 0 && 0 == len) return refuse(kit, err, errlen, "record %d (%s) has no sequence", kit->n, kit->name[kit->n - 1]);
            if (kit->n == FLAPPIE_ADAPTER_MAX_KIT) return refuse(kit, err, errlen, "more than %d records%s", FLAPPIE_ADAPTER_MAX_KIT, NULL);
            const char *e = a + 1;
            while (e < b && !isspace((unsigned char)*e)) e++;
            if (e == a + 1) return refuse(kit, err, errlen, "record %d has no name%s", kit->n + 1, NULL);
            char *name = strndup(a + 1, (size_t)(e - a - 1));
            char *seq = calloc(FLAPPIE_ADAPTER_MAX_LEN + 1, 1);
            if (NULL == name || NULL == seq) { free(name); free(seq); return refuse(kit, err, errlen, "out of memory%.0d%s", 0, NULL); }
            kit->name[kit->n] = name;
            kit->seq[kit->n] = seq;
            kit->n++;
            len = 0;
            if (NULL != strpbrk(name, ",;")) return refuse(kit, err, errlen, "record %d: the name %s holds a ',' or a ';' (they separate the fields of the ah tag)", kit->n, name);
            for (int k = 0; k + 1 < kit->n; k++)
                if (0 == strcmp(kit->name[k], name)) return refuse(kit, err, errlen, "record %d: the name %s occurs twice", kit->n, name);
            continue;
        }
        if (0 == kit->n) return refuse(kit, err, errlen, "text in front of the first record%.0d%s", 0, NULL);
        for (const char *c = a; c < b; c++) {
            const char u = (char)toupper((unsigned char)*c);
            if (NULL == strchr("ACGT", u) || 0 == u) return refuse(kit, err, errlen, "record %d (%s) holds a character that is not one of ACGT", kit->n, kit->name[kit->n - 1]);
            if (len == FLAPPIE_ADAPTER_MAX_LEN) return refuse(kit, err, errlen, "record %d (%s) is longer than 64 bases", kit->n, kit->name[kit->n - 1]);
            kit->seq[kit->n - 1][len++] = u;
        }
    }
    if (0 == kit->n) return refuse(kit, err, errlen, "the kit is empty%.0d%s", 0, NULL);
    if (0 == len) return refuse(kit, err, errlen, "record %d (%s) has no sequence", kit->n, kit->name[kit->n - 1]);
    return kit;
}

flappie_adapter_kit *flappie_adapter_kit_read(const char *path, char *err, size_t errlen) {
    FILE *fh = path ? fopen(path, "r") : NULL;
    if (NULL == fh) return refuse(NULL, err, errlen, "cannot be read%.0d%s", 0, NULL);
    /* (a kit that passes holds at most 32 x (name + 64 bases): a file beyond 1 MiB is refused by size) */
    const size_t cap = (size_t)1 << 20;
    char *text = malloc(cap + 1);
    if (NULL == text) { fclose(fh); return refuse(NULL, err, errlen, "out of memory%.0d%s", 0, NULL); }
    const size_t got = fread(text, 1, cap + 1, fh);
    fclose(fh);
    if (got > cap) { free(text); return refuse(NULL, err, errlen, "larger than 1 MiB: not an adapter kit%.0d%s", 0, NULL); }
    text[got] = 0;
    if (strlen(text) != got) { free(text); return refuse(NULL, err, errlen, "holds a NUL byte: not a FASTA file%.0d%s", 0, NULL); }
    flappie_adapter_kit *kit = flappie_adapter_kit_parse(text, err, errlen);
    free(text);
    return kit;
}

static int record_ok(const ffhip_adapter_header *head, const ffhip_adapter_hit *hits) {
    return NULL != head && head->kept >= 0 && head->kept <= FFHIP_ADAPTER_MAX_HITS && head->kept <= head->nhit && (0 == head->kept || NULL != hits);
}

char *flappie_adapter_tags(const ffhip_adapter_header *head, const ffhip_adapter_hit *hits, const flappie_adapter_kit *kit) {
    if (!record_ok(head, hits) || NULL == kit) return NULL;
    size_t room = 64;
    for (int i = 0; i < head->kept; i++) {
        if (hits[i].pattern < 0 || hits[i].pattern >= kit->n) return NULL;
        room += strlen(kit->name[hits[i].pattern]) + 48;
    }
    char *out = malloc(room);
    if (NULL == out) return NULL;
    size_t a = (size_t)sprintf(out, "an:i:%d\tah:Z:", (int)head->nhit);
    for (int i = 0; i < head->kept; i++)
        a += (size_t)sprintf(out + a, "%s,%c,%d,%d,%d;", kit->name[hits[i].pattern], hits[i].orientation ? '-' : '+', (int)hits[i].start, (int)hits[i].end, (int)hits[i].dist);
    return out;
}

int flappie_adapter_trim(const ffhip_adapter_header *head, const ffhip_adapter_hit *hits, size_t length, int window, size_t *from, size_t *to) {
    size_t lo = 0, hi = length;
    if (record_ok(head, hits)) {
        const long W = window > 0 ? window : 0, len = (long)length;
        for (int i = 0; i < head->kept; i++) {
            if (hits[i].end <= W && hits[i].end > 0 && (size_t)hits[i].end > lo) lo = (size_t)hits[i].end;
            if (hits[i].start >= len - W && hits[i].start >= 0 && (size_t)hits[i].start < hi) hi = (size_t)hits[i].start;
        }
    }
    const int crossed = (lo > 0 || hi < length) && lo >= hi;
    if (from) *from = crossed ? 0 : lo;
    if (to) *to = crossed ? 0 : hi;
    return crossed;
}

int flappie_adapter_split(const ffhip_adapter_header *head, const ffhip_adapter_hit *hits, size_t length, int window, size_t min_length, size_t clip_from, size_t clip_to,
                          flappie_adapter_piece pieces[FLAPPIE_ADAPTER_MAX_PIECES], int *npiece, int *ndropped) {
    int np = 0, nd = 0, mode = FLAPPIE_SPLIT_WHOLE;
    if (clip_to > length) clip_to = length;
    if (record_ok(head, hits) && head->nhit > FFHIP_ADAPTER_MAX_HITS) mode = FLAPPIE_SPLIT_OVERFLOW;
    else {
        size_t lo = 0, hi = length;
        int crossed = flappie_adapter_trim(head, hits, length, window, &lo, &hi);
        if (!crossed) {                   /* within the clip: the larger cut at each end wins */
            if (clip_from > lo) lo = clip_from;
            if (clip_to < hi) hi = clip_to;
            if (lo >= hi && length > 0) { crossed = 1; lo = hi = 0; }
        }
        const long W = window > 0 ? window : 0, len = (long)length;
        int interior = 0;
        if (record_ok(head, hits)) for (int i = 0; i < head->kept; i++) if (!(hits[i].end <= W || hits[i].start >= len - W)) interior++;
        if (0 == interior) { pieces[0].from = lo; pieces[0].to = hi; np = 1; }
        else {
            /* the kept hits are ordered by end, not by start: walk the range and jump over whatever covers the position */
            mode = FLAPPIE_SPLIT_SPLIT;
            size_t at = lo;
            while (at < hi) {
                size_t cover = at, next = hi;             /* the furthest end of a hit that covers `at`; else the nearest start behind it */
                for (int i = 0; i < head->kept; i++) {
                    const size_t s = hits[i].start > 0 ? (size_t)hits[i].start : 0, e = hits[i].end > 0 ? (size_t)hits[i].end : 0;
                    if (s <= at && e > cover) cover = e;
                    if (s > at && s < next) next = s;
                }
                if (cover > at) { at = cover; continue; }
                if (next - at >= min_length) { pieces[np].from = at; pieces[np].to = next; np++; } else nd++;
                at = next;
            }
        }
    }
    if (npiece) *npiece = np;
    if (ndropped) *ndropped = nd;
    return mode;
}

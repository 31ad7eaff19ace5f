/*  flappie_barcodes.c -- the host side of flappie --barcodes (include/flappie_barcodes.h): the kit's parser, the tags of a record, the trim.
 *  The classification is the GPU's (k_barcodes, FFHIP_RUN_BARCODES).
 */
#include <ctype.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_barcodes.h"

void flappie_barcode_kit_free(flappie_barcode_kit *kit) {
    if (NULL == kit) return;
    for (int k = 0; k < kit->n; k++) { if (kit->name) free(kit->name[k]); if (kit->seq) free(kit->seq[k]); }
    free(kit->name);
    free(kit->seq);
    free(kit);
}

static flappie_barcode_kit *refuse(flappie_barcode_kit *kit, char *err, size_t errlen, const char *fmt, int a, const char *s) {
    if (err && errlen) snprintf(err, errlen, fmt, a, s ? s : "");
    flappie_barcode_kit_free(kit);
    return NULL;
}

flappie_barcode_kit *flappie_barcode_kit_parse(const char *text, char *err, size_t errlen) {
    if (NULL == text) return refuse(NULL, err, errlen, "no kit text%.0d%s", 0, NULL);
    flappie_barcode_kit *kit = calloc(1, sizeof(*kit));
    if (kit) { kit->name = calloc(FLAPPIE_BARCODE_MAX_KIT, sizeof(char *)); kit->seq = calloc(FLAPPIE_BARCODE_MAX_KIT, sizeof(char *)); }
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
            if (kit->n == FLAPPIE_BARCODE_MAX_KIT) return refuse(kit, err, errlen, "more than %d records%s", FLAPPIE_BARCODE_MAX_KIT, NULL);
            const char *e = a + 1;
            while (e < b && !isspace((unsigned char)*e)) e++;
            if (e == a + 1) return refuse(kit, err, errlen, "record %d has no name%s", kit->n + 1, NULL);
            char *name = strndup(a + 1, (size_t)(e - a - 1));
            char *seq = calloc(FLAPPIE_BARCODE_MAX_LEN + 1, 1);
            if (NULL == name || NULL == seq) { free(name); free(seq); return refuse(kit, err, errlen, "out of memory%.0d%s", 0, NULL); }
            kit->name[kit->n] = name;
            kit->seq[kit->n] = seq;
            kit->n++;
            len = 0;
            for (int k = 0; k + 1 < kit->n; k++)
                if (0 == strcmp(kit->name[k], name)) return refuse(kit, err, errlen, "record %d: the name %s occurs twice", kit->n, name);
            continue;
        }
        if (0 == kit->n) return refuse(kit, err, errlen, "text in front of the first record%.0d%s", 0, NULL);
        for (const char *c = a; c < b; c++) {
            const char u = (char)toupper((unsigned char)*c);
            if (NULL == strchr("ACGT", u) || 0 == u) return refuse(kit, err, errlen, "record %d (%s) holds a character that is not one of ACGT", kit->n, kit->name[kit->n - 1]);
            if (len == FLAPPIE_BARCODE_MAX_LEN) return refuse(kit, err, errlen, "record %d (%s) is longer than 128 bases", kit->n, kit->name[kit->n - 1]);
            kit->seq[kit->n - 1][len++] = u;
        }
    }
    if (0 == kit->n) return refuse(kit, err, errlen, "the kit is empty%.0d%s", 0, NULL);
    if (0 == len) return refuse(kit, err, errlen, "record %d (%s) has no sequence", kit->n, kit->name[kit->n - 1]);
    kit->lmin = FLAPPIE_BARCODE_MAX_LEN;
    for (int k = 0; k < kit->n; k++) { const int l = (int)strlen(kit->seq[k]); if (l < kit->lmin) kit->lmin = l; }
    return kit;
}

flappie_barcode_kit *flappie_barcode_kit_read(const char *path, char *err, size_t errlen) {
    FILE *fh = path ? fopen(path, "r") : NULL;
    if (NULL == fh) return refuse(NULL, err, errlen, "cannot be read%.0d%s", 0, NULL);
    /* (a kit that passes holds at most 128 x (name + 128 bases): a file beyond 1 MiB is refused by size) */
    const size_t cap = (size_t)1 << 20;
    char *text = malloc(cap + 1);
    if (NULL == text) { fclose(fh); return refuse(NULL, err, errlen, "out of memory%.0d%s", 0, NULL); }
    const size_t got = fread(text, 1, cap + 1, fh);
    fclose(fh);
    if (got > cap) { free(text); return refuse(NULL, err, errlen, "larger than 1 MiB: not a barcode kit%.0d%s", 0, NULL); }
    text[got] = 0;
    if (strlen(text) != got) { free(text); return refuse(NULL, err, errlen, "holds a NUL byte: not a FASTA file%.0d%s", 0, NULL); }
    flappie_barcode_kit *kit = flappie_barcode_kit_parse(text, err, errlen);
    free(text);
    return kit;
}

char *flappie_barcode_tags(const ffhip_barcode_call *call, const flappie_barcode_kit *kit) {
    if (NULL == call || NULL == kit || call->best >= kit->n) return NULL;
    const char *name = call->best >= 0 ? kit->name[call->best] : "unclassified";
    char *out = malloc(strlen(name) + 96);
    if (NULL == out) return NULL;
    sprintf(out, "BC:Z:%s\tbd:i:%d\tbn:i:%d\tbp:B:s,%d,%d", name, (int)call->best_dist, (int)call->second_dist, (int)call->front_end, (int)call->rear_end);
    return out;
}

int flappie_barcode_trim(const ffhip_barcode_call *call, size_t length, size_t *from, size_t *to) {
    size_t lo = 0, cut = 0;
    if (NULL != call && call->best >= 0) {
        if ((call->ends & 1) && call->front_end > 0) lo = (size_t)call->front_end;
        if ((call->ends & 2) && call->rear_end > 0) cut = (size_t)call->rear_end;
    }
    const int crossed = lo + cut > 0 && lo + cut >= length;      /* (an empty call that loses nothing is not a crossing) */
    if (from) *from = crossed ? 0 : lo;
    if (to) *to = crossed ? 0 : length - cut;
    return crossed;
}

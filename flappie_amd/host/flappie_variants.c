/*  flappie_variants.c -- the reader of flappie --remap-variants' file and the lines of --remap-variants-out (include/flappie_variants.h) */
#include <ctype.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_variants.h"

#define MAX_ALLELE 16

static const char *const kind_text[FLAPPIE_VARIANTS_KINDS] = {
    "is malformed (name, pos, ref and alt separated by tabs; pos a whole number from 0; not both alleles empty; an edit that leaves a base)",
    "holds a letter outside the model's alphabet",
    "has an allele longer than 16",
    "names no record of --remap's file that can be used",
    "lies beyond its record",
    "has a ref that is not the record's letters at pos",
};

const char *flappie_variants_kind(int kind) { return (kind >= 0 && kind < FLAPPIE_VARIANTS_KINDS) ? kind_text[kind] : ""; }

static void set_why(char *err, size_t errlen, const char *why) {
    if (err && errlen) snprintf(err, errlen, "%s", why);
}

void flappie_variants_free(flappie_variants *vs) {
    if (NULL == vs) return;
    free(vs->rec);
    free(vs->var);
    free(vs->first);
    free(vs->idx);
    free(vs);
}

/* an allele's codes from its field [s, s + n): 0 and *len, or the kind it is skipped for */
static int allele(const char *s, size_t n, const char *alphabet, uint8_t *codes, int *len) {
    *len = 0;
    if (0 == n) return FLAPPIE_VARIANTS_MALFORMED;
    if (1 == n && '-' == s[0]) return -1;
    if (n > MAX_ALLELE) return FLAPPIE_VARIANTS_LONG;
    for (size_t i = 0; i < n; i++) {
        const int c = toupper((unsigned char)s[i]);
        const char *at = c ? strchr(alphabet, c) : NULL;
        if (NULL == at) return FLAPPIE_VARIANTS_LETTER;
        codes[i] = (uint8_t)(at - alphabet);
    }
    *len = (int)n;
    return -1;
}

/* one line [s, s + n) (no line end): -1 and the variant, or the kind it is skipped for */
static int parse_line(const char *s, size_t n, const flappie_remap_refs *refs, const char *alphabet, int *rec, ffhip_variant *v) {
    const char *f[4];
    size_t fl[4];
    int nf = 0;
    size_t at = 0;
    for (size_t i = 0; i <= n; i++) {
        if (i < n && '\t' != s[i]) continue;
        if (nf == 4) return FLAPPIE_VARIANTS_MALFORMED;
        f[nf] = s + at; fl[nf] = i - at; nf++;
        at = i + 1;
    }
    if (4 != nf || 0 == fl[0] || 0 == fl[1] || fl[1] > 18) return FLAPPIE_VARIANTS_MALFORMED;
    unsigned long long pos = 0;
    for (size_t i = 0; i < fl[1]; i++) {
        if (f[1][i] < '0' || f[1][i] > '9') return FLAPPIE_VARIANTS_MALFORMED;
        pos = pos * 10 + (unsigned long long)(f[1][i] - '0');
    }
    memset(v, 0, sizeof *v);
    uint8_t refc[MAX_ALLELE];
    int nref = 0, nalt = 0;
    int kind = allele(f[2], fl[2], alphabet, refc, &nref);
    if (kind >= 0) return kind;
    if ((kind = allele(f[3], fl[3], alphabet, v->alt, &nalt)) >= 0) return kind;
    if (0 == nref + nalt) return FLAPPIE_VARIANTS_MALFORMED;
    char name[256];
    if (fl[0] >= sizeof name) return FLAPPIE_VARIANTS_NO_RECORD;
    memcpy(name, f[0], fl[0]);
    name[fl[0]] = '\0';
    const int k = flappie_remap_refs_find(refs, name, name);
    if (k < 0 || refs->bad[k] || NULL == refs->codes[k] || 0 == refs->len[k]) return FLAPPIE_VARIANTS_NO_RECORD;
    const size_t L = refs->len[k];
    if (pos > L || pos + (unsigned)nref > L || pos > 0x7fffffffull) return FLAPPIE_VARIANTS_BEYOND;
    if (0 != memcmp(refs->codes[k] + pos, refc, (size_t)nref)) return FLAPPIE_VARIANTS_REF_MISMATCH;
    if (L - (size_t)nref + (size_t)nalt < 1) return FLAPPIE_VARIANTS_MALFORMED;
    v->pos = (int32_t)pos; v->nref = (uint8_t)nref; v->nalt = (uint8_t)nalt;
    *rec = k;
    return -1;
}

flappie_variants *flappie_variants_parse(const char *text, const flappie_remap_refs *refs, const char *alphabet, char *err, size_t errlen) {
    if (NULL == text || NULL == refs || NULL == alphabet) { set_why(err, errlen, "no text, or no records to hold it against"); return NULL; }
    flappie_variants *vs = calloc(1, sizeof *vs);
    if (NULL == vs) { set_why(err, errlen, "out of memory"); return NULL; }
    size_t cap = 0, line = 0;
    vs->nrec = refs->n;
    for (const char *s = text; *s;) {
        const char *e = strchr(s, '\n');
        size_t n = e ? (size_t)(e - s) : strlen(s);
        const char *next = e ? e + 1 : s + n;
        if (n && '\r' == s[n - 1]) n--;
        line++;
        if (n && '#' != s[0]) {
            int rec = -1;
            ffhip_variant v;
            const int kind = parse_line(s, n, refs, alphabet, &rec, &v);
            if (kind >= 0) {
                if (0 == vs->skipped[kind]++) {
                    const size_t m = n < sizeof vs->skipped_text[kind] - 1 ? n : sizeof vs->skipped_text[kind] - 1;
                    vs->skipped_line[kind] = line;
                    memcpy(vs->skipped_text[kind], s, m);
                    vs->skipped_text[kind][m] = '\0';
                }
            } else {
                if (vs->n == cap) {
                    const size_t ncap = cap ? 2 * cap : 64;
                    int *nr = realloc(vs->rec, ncap * sizeof *nr);
                    if (nr) vs->rec = nr;
                    ffhip_variant *nv = realloc(vs->var, ncap * sizeof *nv);
                    if (nv) vs->var = nv;
                    if (NULL == nr || NULL == nv) { set_why(err, errlen, "out of memory"); flappie_variants_free(vs); return NULL; }
                    cap = ncap;
                }
                vs->rec[vs->n] = rec;
                vs->var[vs->n] = v;
                vs->n++;
            }
        }
        s = next;
    }
    /* the variants by record, in file order within one: a counting sort */
    vs->first = calloc((size_t)vs->nrec + 2, sizeof *vs->first);
    vs->idx = calloc(vs->n ? vs->n : 1, sizeof *vs->idx);
    if (NULL == vs->first || NULL == vs->idx) { set_why(err, errlen, "out of memory"); flappie_variants_free(vs); return NULL; }
    for (size_t i = 0; i < vs->n; i++) vs->first[vs->rec[i] + 2]++;
    for (int k = 0; k < vs->nrec; k++) vs->first[k + 2] += vs->first[k + 1];
    for (size_t i = 0; i < vs->n; i++) vs->idx[vs->first[vs->rec[i] + 1]++] = i;      /* (first[k + 1] ends as the end of record k: first[k] is its start) */
    return vs;
}

flappie_variants *flappie_variants_read(const char *path, const flappie_remap_refs *refs, const char *alphabet, char *err, size_t errlen) {
    FILE *fh = path ? fopen(path, "rb") : NULL;
    if (NULL == fh) { set_why(err, errlen, "cannot be read"); return NULL; }
    size_t cap = 1 << 16, n = 0;
    char *text = malloc(cap);
    while (text) {
        n += fread(text + n, 1, cap - n - 1, fh);
        if (n < cap - 1) break;
        char *more = realloc(text, cap *= 2);
        if (NULL == more) { free(text); text = NULL; }
        else text = more;
    }
    const int bad = ferror(fh);
    fclose(fh);
    if (NULL == text || bad) { free(text); set_why(err, errlen, text ? "cannot be read" : "out of memory"); return NULL; }
    for (size_t i = 0; i < n; i++) if ('\0' == text[i]) text[i] = ' ';      /* (a NUL would end the text early: the line becomes malformed instead) */
    text[n] = '\0';
    flappie_variants *vs = flappie_variants_parse(text, refs, alphabet, err, errlen);
    free(text);
    return vs;
}

size_t flappie_variants_of(const flappie_variants *vs, int rec, ffhip_variant *out) {
    if (NULL == vs || rec < 0 || rec >= vs->nrec) return 0;
    const size_t a = vs->first[rec], e = vs->first[rec + 1];
    if (out) for (size_t i = a; i < e; i++) out[i - a] = vs->var[vs->idx[i]];
    return e - a;
}

static void put_allele(FILE *out, const uint8_t *codes, size_t n, const char *alphabet) {
    if (0 == n) fputc('-', out);
    for (size_t i = 0; i < n; i++) fputc(alphabet[codes[i]], out);
}

int flappie_variants_write(FILE *out, const char *name, const uint8_t *codes, size_t L, const char *alphabet, const ffhip_variant *var, const ffhip_variant_call *vc, size_t n) {
    const size_t na = strlen(alphabet);
    for (size_t i = 0; i < n; i++) {
        if (vc[i].index < 0 || (size_t)vc[i].index >= n) return -1;
        const ffhip_variant *v = var + vc[i].index;
        if (v->pos < 0 || v->nref > MAX_ALLELE || v->nalt > MAX_ALLELE || (size_t)v->pos + v->nref > L) return -1;
        for (int j = 0; j < v->nalt; j++) if (v->alt[j] >= na) return -1;
        const double ref = (double)vc[i].ref, alt = (double)vc[i].alt;
        const double diff = (isinf(alt) && alt < 0) ? ((isinf(ref) && ref < 0) ? 0.0 : INFINITY) : ref - alt;
        fprintf(out, "%s\t%d\t", name, (int)v->pos);
        put_allele(out, codes + v->pos, v->nref, alphabet);
        fputc('\t', out);
        put_allele(out, v->alt, v->nalt, alphabet);
        fprintf(out, "\t%d\t%.9g\t%.9g\t%.9g\n", (int)vc[i].nblock, ref, alt, diff);
    }
    return 0;
}

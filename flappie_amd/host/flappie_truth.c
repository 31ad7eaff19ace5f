/*  flappie_truth.c -- the host side of flappie --truth (include/flappie_truth.h): the CIGAR of a read's ops, the line of acc.tsv, the summary.
 *  The alignment is the GPU's (k_truth, FFHIP_RUN_TRUTH).
 */
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_truth.h"

double flappie_truth_identity(const flappie_truth_rec *rec) {
    const long long cols = (long long)rec->n_match + rec->n_mismatch + rec->n_ins + rec->n_del;
    return cols > 0 ? (double)rec->n_match / (double)cols : 0.0;
}

long flappie_truth_write_cigar(FILE *out, const uint8_t *ops, size_t nops) {
    static const char letter[4] = { '=', 'X', 'I', 'D' };
    if (0 == nops || NULL == ops) return fputc('*', out) == EOF ? -1 : 1;
    for (size_t i = 0; i < nops; i++) if (ops[i] > 3) return -1;
    long wrote = 0;
    for (size_t i = 0; i < nops; ) {
        size_t e = i + 1;
        while (e < nops && ops[e] == ops[i]) e++;
        wrote += fprintf(out, "%zu%c", e - i, letter[ops[i]]);
        i = e;
    }
    return wrote;
}

int flappie_truth_write_fields(FILE *out, const char *name, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops) {
    if (1 != rec->status) {
        fprintf(out, "%s\t%d\t%zu\t%zu\t%d\t*\t*\t*\t*\t*\t*\t*\t*", name, rec->status, rec->n, rec->m, rec->band);
        return 0;
    }
    size_t cnt[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < nops; i++) { if (NULL == ops || ops[i] > 3) return -1; cnt[ops[i]]++; }
    if (cnt[0] != (size_t)rec->n_match || cnt[1] != (size_t)rec->n_mismatch || cnt[2] != (size_t)rec->n_ins || cnt[3] != (size_t)rec->n_del ||
        cnt[0] + cnt[1] + cnt[2] != rec->n || cnt[0] + cnt[1] + cnt[3] != rec->m)
        return -1;
    fprintf(out, "%s\t%d\t%zu\t%zu\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%.6f\t", name, rec->status, rec->n, rec->m, rec->band, rec->maxdev, rec->dist, rec->n_match, rec->n_mismatch,
            rec->n_ins, rec->n_del, flappie_truth_identity(rec));
    flappie_truth_write_cigar(out, ops, nops);
    return 0;
}

int flappie_truth_write_line(FILE *out, const char *name, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops) {
    if (0 != flappie_truth_write_fields(out, name, rec, ops, nops)) return -1;
    fputc('\n', out);
    return 0;
}

int flappie_truth_summary_add(flappie_truth_summary *sum, const flappie_truth_rec *rec) {
    if (NULL == rec) { sum->no_record++; return 0; }
    if (1 != rec->status) { sum->not_aligned++; return 0; }
    if (sum->nid == sum->cap) {
        const size_t cap = sum->cap ? 2 * sum->cap : 1024;
        double *id = realloc(sum->identity, cap * sizeof(double));
        if (NULL == id) return -1;
        sum->identity = id; sum->cap = cap;
    }
    sum->identity[sum->nid++] = flappie_truth_identity(rec);
    sum->aligned++;
    if (rec->maxdev == rec->band) sum->band_touched++;
    sum->matches += (unsigned long long)rec->n_match;
    sum->columns += (unsigned long long)rec->n_match + (unsigned long long)rec->n_mismatch + (unsigned long long)rec->n_ins + (unsigned long long)rec->n_del;
    return 0;
}

double flappie_truth_summary_pooled(const flappie_truth_summary *sum) { return sum->columns ? (double)sum->matches / (double)sum->columns : 0.0; }

static int by_value(const void *x, const void *y) {
    const double a = *(const double *)x, b = *(const double *)y;
    return (a > b) - (a < b);
}

double flappie_truth_summary_median(flappie_truth_summary *sum) {
    if (0 == sum->nid) return 0.0;
    qsort(sum->identity, sum->nid, sizeof(double), by_value);
    const size_t h = sum->nid / 2;
    return (sum->nid & 1) ? sum->identity[h] : 0.5 * (sum->identity[h - 1] + sum->identity[h]);
}

void flappie_truth_summary_print(FILE *out, flappie_truth_summary *sum) {
    fprintf(out, "truth\taligned\t%llu\ntruth\tnot_aligned\t%llu\ntruth\tno_record\t%llu\ntruth\tband_touched\t%llu\ntruth\tpooled_identity\t%.6f\ntruth\tmedian_identity\t%.6f\n",
            sum->aligned, sum->not_aligned, sum->no_record, sum->band_touched, flappie_truth_summary_pooled(sum), flappie_truth_summary_median(sum));
}

void flappie_truth_summary_free(flappie_truth_summary *sum) {
    free(sum->identity);
    memset(sum, 0, sizeof(*sum));
}

/*  flappie_pileup.c -- the host side of flappie --map-pileup (include/flappie_pileup.h): the table of per-position counts and the summary.  The counters are the
 *  GPU's (k_pileup).
 */
#include "../../include/flappie_pileup.h"

int flappie_pileup_write(FILE *out, const flappie_map_ref *ref, const uint32_t *counts, unsigned long long *covered) {
    if (NULL == out || NULL == ref || NULL == counts) return -1;
    size_t P = 0, at = 0;
    unsigned long long cov = 0;
    for (int k = 0; k < ref->n; k++) P += ref->len[k];
    for (int k = 0; k < ref->n; k++) {
        for (size_t x = 0; x < ref->len[k]; x++, at++) {
            unsigned long long depth = 0;
            for (int o = 0; o < 2; o++) for (int c = 0; c < 5; c++) depth += counts[(size_t)(6 * o + c) * P + at];
            cov += depth >= 1;
            const char r = ref->seq[k][x];
            fprintf(out, "%s\t%zu\t%c\t%llu", ref->name[k], x, (r >= 'a' && r <= 'z') ? (char)(r - 'a' + 'A') : r, depth);
            for (int pl = 0; pl < FFHIP_PILEUP_PLANES; pl++) fprintf(out, "\t%u", (unsigned)counts[(size_t)pl * P + at]);
            fputc('\n', out);
        }
    }
    if (covered) *covered = cov;
    return 0;
}

void flappie_pileup_summary_print(FILE *out, const ffhip_pileup_totals *t, unsigned long long positions, unsigned long long covered) {
    fprintf(out, "pileup\treads\t%llu\npileup\tskipped\t%llu\npileup\tpositions\t%llu\npileup\tcovered\t%llu\npileup\tmatch\t%llu\npileup\tmismatch\t%llu\n"
                 "pileup\tdel\t%llu\npileup\tins\t%llu\npileup\tedge_ins\t%llu\n",
            (unsigned long long)t->reads, (unsigned long long)t->skipped, positions, covered, (unsigned long long)t->match, (unsigned long long)t->mismatch,
            (unsigned long long)t->del, (unsigned long long)t->ins, (unsigned long long)t->edge_ins);
}

/*  flappie_errprofile.c -- the host side of flappie --truth-errors (include/flappie_errprofile.h): the table of the run's error profile and the summary.  The
 *  counters are the GPU's (k_errprofile).  Integers only.
 */
#include "../../include/flappie_errprofile.h"

int flappie_errprofile_write(FILE *out, const uint64_t *counts) {
    if (NULL == out || NULL == counts) return -1;
    static const char letter[] = "ACGT-";
    const uint64_t *sub = counts + FFHIP_ERRPROFILE_SUB, *ins = counts + FFHIP_ERRPROFILE_INS, *qual = counts + FFHIP_ERRPROFILE_QUAL,
                   *ctx = counts + FFHIP_ERRPROFILE_CTX, *hp = counts + FFHIP_ERRPROFILE_HP;
    for (int t = 0; t < 4; t++)
        for (int c = 0; c < 5; c++) fprintf(out, "sub\t%c\t%c\t%llu\n", letter[t], letter[c], (unsigned long long)sub[5 * t + c]);
    for (int c = 0; c < 4; c++) fprintf(out, "ins\t%c\t%llu\n", letter[c], (unsigned long long)ins[c]);
    for (int q = 0; q < 94; q++)
        fprintf(out, "qual\t%d\t%llu\t%llu\t%llu\n", q, (unsigned long long)qual[3 * q], (unsigned long long)qual[3 * q + 1], (unsigned long long)qual[3 * q + 2]);
    for (int w = 0; w < 1024; w++) {
        const uint64_t *c = ctx + 4 * w;
        if (0 == (c[0] | c[1] | c[2] | c[3])) continue;
        char mer[6];
        for (int d = 0; d < 5; d++) mer[d] = letter[(w >> (2 * (4 - d))) & 3];
        mer[5] = '\0';
        fprintf(out, "ctx\t%s\t%llu\t%llu\t%llu\t%llu\n", mer, (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3]);
    }
    for (int b = 0; b < 4; b++)
        for (int r = 0; r < FFHIP_ERRPROFILE_HP_MAX_RUN; r++)
            for (int c = 0; c <= FFHIP_ERRPROFILE_HP_MAX_CALLED; c++) {
                const uint64_t v = hp[(b * FFHIP_ERRPROFILE_HP_MAX_RUN + r) * (FFHIP_ERRPROFILE_HP_MAX_CALLED + 1) + c];
                if (v) fprintf(out, "hp\t%c\t%d\t%d\t%llu\n", letter[b], r + 1, c, (unsigned long long)v);
            }
    return 0;
}

void flappie_errprofile_summary_print(FILE *out, const ffhip_errprofile_totals *t) {
    fprintf(out, "errors\treads\t%llu\nerrors\tskipped\t%llu\nerrors\tmatch\t%llu\nerrors\tmismatch\t%llu\nerrors\tdel\t%llu\nerrors\tins\t%llu\nerrors\tedge_ins\t%llu\n"
                 "errors\tctx_sites\t%llu\nerrors\thp_runs\t%llu\nerrors\thp_long\t%llu\nerrors\thp_wide\t%llu\nerrors\treserved\t%llu\n",
            (unsigned long long)t->reads, (unsigned long long)t->skipped, (unsigned long long)t->match, (unsigned long long)t->mismatch, (unsigned long long)t->del,
            (unsigned long long)t->ins, (unsigned long long)t->edge_ins, (unsigned long long)t->ctx_sites, (unsigned long long)t->hp_runs, (unsigned long long)t->hp_long,
            (unsigned long long)t->hp_wide, (unsigned long long)t->reserved);
}

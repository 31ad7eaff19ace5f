/*  flappie_modpileup.c -- the host side of flappie --map-mods (include/flappie_modpileup.h): the bedMethyl table, the histogram's file and the summary.  The
 *  counters are the GPU's (k_modpileup).
 */
#include "../../include/flappie_modpileup.h"

static char upper(char r) { return (r >= 'a' && r <= 'z') ? (char)(r - 'a' + 'A') : r; }

int flappie_modpileup_write(FILE *out, const flappie_map_ref *ref, const uint32_t *counts, int motif, int combine, unsigned long long *rows) {
    if (NULL == out || NULL == ref || NULL == counts) return -1;
    if ((motif != FLAPPIE_MODS_MOTIF_CG && motif != FLAPPIE_MODS_MOTIF_C) || (combine && motif != FLAPPIE_MODS_MOTIF_CG)) return -1;
    size_t P = 0, off = 0;
    unsigned long long written = 0;
    for (int k = 0; k < ref->n; k++) P += ref->len[k];
    for (int k = 0; k < ref->n; off += ref->len[k], k++) {
        const char *s = ref->seq[k];
        const size_t M = ref->len[k];
        for (size_t f = 0; f < M; f++) {
            const char r = upper(s[f]);
            for (int o = 0; o < (combine ? 1 : 2); o++) {
                if (r != (o ? 'G' : 'C')) continue;
                if (motif == FLAPPIE_MODS_MOTIF_CG && !(o ? (f >= 1 && upper(s[f - 1]) == 'C') : (f + 1 < M && upper(s[f + 1]) == 'G'))) continue;
                unsigned long long c[5];
                for (int x = 0; x < 5; x++) {
                    c[x] = counts[(size_t)(5 * o + x) * P + off + f];
                    if (combine) c[x] += counts[(size_t)(5 + x) * P + off + f + 1];       /* (the G behind a C of the motif: f + 1 < M) */
                }
                if (c[0] + c[1] + c[2] + c[3] + c[4] < 1) continue;
                const unsigned long long nv = c[0] + c[1];
                fprintf(out, "%s\t%zu\t%zu\tm\t%llu\t%c\t%zu\t%zu\t255,0,0\t%llu\t", ref->name[k], f, f + 1, nv, combine ? '.' : (o ? '-' : '+'), f, f + 1, nv);
                if (nv) fprintf(out, "%.2f", 100.0 * (double)c[0] / (double)nv); else fputs("0.00", out);
                fprintf(out, "\t%llu\t%llu\t0\t%llu\t%llu\t%llu\t0\n", c[0], c[1], c[4], c[2], c[3]);
                written++;
            }
        }
    }
    if (rows) *rows = written;
    return 0;
}

int flappie_modpileup_hist_write(FILE *out, const uint64_t *hist) {
    if (NULL == out || NULL == hist) return -1;
    for (int v = 0; v < 256; v++) fprintf(out, "%d\t%llu\n", v, (unsigned long long)hist[v]);
    return 0;
}

void flappie_modpileup_summary_print(FILE *out, const ffhip_modpileup_totals *t, unsigned long long rows) {
    fprintf(out, "mods_pileup\treads\t%llu\nmods_pileup\tskipped\t%llu\nmods_pileup\tsites\t%llu\nmods_pileup\tmod\t%llu\nmods_pileup\tcanon\t%llu\n"
                 "mods_pileup\tfail\t%llu\nmods_pileup\tdiff\t%llu\nmods_pileup\tdel\t%llu\nmods_pileup\trows\t%llu\n",
            (unsigned long long)t->reads, (unsigned long long)t->skipped, (unsigned long long)t->sites, (unsigned long long)t->mod, (unsigned long long)t->canon,
            (unsigned long long)t->fail, (unsigned long long)t->diff, (unsigned long long)t->del, rows);
}

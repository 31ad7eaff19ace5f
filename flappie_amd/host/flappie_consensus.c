/*  flappie_consensus.c -- the host side of flappie --map-consensus (include/flappie_consensus.h): the FASTA file, the table of changes and the summary.  The
 *  counters and the cells are the GPU's (k_consensus, k_consensus_call).
 */
#include "../../include/flappie_consensus.h"

enum { CONSENSUS_LINE = 70 };

static int cell_letters(const ffhip_consensus_cell *c) { return c->n > sizeof c->s ? (int)sizeof c->s : (int)c->n; }

int flappie_consensus_write(FILE *out, const flappie_map_ref *ref, const ffhip_consensus_cell *cells, flappie_consensus_stats *stats) {
    if (NULL == out || NULL == ref || NULL == cells) return -1;
    flappie_consensus_stats st = { 0, 0, 0, 0, 0, 0, 0 };
    size_t at = 0;
    for (int k = 0; k < ref->n; k++) {
        fprintf(out, ">%s\n", ref->name[k]);
        size_t col = 0, written = 0;
        for (size_t x = 0; x < ref->len[k]; x++, at++) {
            const ffhip_consensus_cell *c = cells + at;
            const int n = cell_letters(c), kind = c->what & 3;
            for (int i = 0; i < n; i++) {
                fputc(c->s[i], out);
                written++;
                if (++col == CONSENSUS_LINE) { fputc('\n', out); col = 0; }
            }
            st.positions++;
            if (kind == FFHIP_CONSENSUS_LOW) { st.low_depth++; continue; }
            st.called++;
            st.same += kind == FFHIP_CONSENSUS_SAME; st.sub += kind == FFHIP_CONSENSUS_SUB; st.del += kind == FFHIP_CONSENSUS_DEL;
            if (c->what & FFHIP_CONSENSUS_INS) st.ins += (unsigned long long)(n - (kind != FFHIP_CONSENSUS_DEL));
        }
        if (col || 0 == written) fputc('\n', out);
    }
    if (stats) *stats = st;
    return 0;
}

int flappie_consensus_changes_write(FILE *out, const flappie_map_ref *ref, const ffhip_consensus_cell *cells, const uint32_t *counts) {
    if (NULL == out || NULL == ref || NULL == cells || NULL == counts) return -1;
    size_t P = 0, at = 0;
    for (int k = 0; k < ref->n; k++) P += ref->len[k];
    for (int k = 0; k < ref->n; k++) {
        for (size_t x = 0; x < ref->len[k]; x++, at++) {
            const ffhip_consensus_cell *c = cells + at;
            if (c->what == FFHIP_CONSENSUS_LOW || c->what == FFHIP_CONSENSUS_SAME) continue;
            const int n = cell_letters(c), kind = c->what & 3;
            const char r0 = ref->seq[k][x], r = (r0 >= 'a' && r0 <= 'z') ? (char)(r0 - 'a' + 'A') : r0;
            const char w = kind == FFHIP_CONSENSUS_DEL ? '-' : c->s[0];       /* the winner's plane: its letter, or del */
            const int plane = w == 'A' ? 0 : w == 'C' ? 1 : w == 'G' ? 2 : w == 'T' ? 3 : 4;
            unsigned long long first = 0;
            if (c->what & FFHIP_CONSENSUS_INS) for (int b = 0; b < 4; b++) first += counts[(size_t)(5 + b) * P + at];
            fprintf(out, "%s\t%zu\t%c\t", ref->name[k], x, r);
            if (n) fwrite(c->s, 1, (size_t)n, out); else fputc('-', out);
            fprintf(out, "\t%u\t%u\t%llu\n", (unsigned)c->depth, (unsigned)counts[(size_t)plane * P + at], first);
        }
    }
    return 0;
}

void flappie_consensus_summary_print(FILE *out, const ffhip_consensus_totals *t, const flappie_consensus_stats *st) {
    fprintf(out, "consensus\treads\t%llu\nconsensus\tskipped\t%llu\nconsensus\tpositions\t%llu\nconsensus\tcalled\t%llu\nconsensus\tlow_depth\t%llu\n"
                 "consensus\tsame\t%llu\nconsensus\tsub\t%llu\nconsensus\tdel\t%llu\nconsensus\tins\t%llu\nconsensus\tlong_ins\t%llu\nconsensus\tedge_ins\t%llu\n",
            (unsigned long long)t->reads, (unsigned long long)t->skipped, st->positions, st->called, st->low_depth, st->same, st->sub, st->del, st->ins,
            (unsigned long long)t->long_ins, (unsigned long long)t->edge_ins);
}

/*  flappie_align.c -- the host side of flappie --truth-from-map (include/flappie_align.h): the line of acc.tsv with the place behind the alignment, and the aligned
 *  SAM file.  Map and alignment are the GPU's (k_map_scan, k_map_finish, k_map_stretch, k_truth).
 */
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_align.h"

int flappie_align_write_acc_line(FILE *out, const char *name, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops, const ffhip_map_call *map,
                                 const flappie_map_ref *ref) {
    if (NULL == out || NULL == name || NULL == rec || NULL == map || NULL == ref || 1 != map->status) return -1;
    int k = 0;
    char o = '+';
    long a = 0, b = 0;
    if (0 != flappie_map_forward(ref, map->q, map->tstart, map->tend, &k, &o, &a, &b)) return -1;
    if (1 == rec->status) {                /* (flappie_truth_write_fields writes nothing when it refuses: the same test, ahead of it) */
        size_t cnt[4] = { 0, 0, 0, 0 };
        for (size_t i = 0; i < nops; i++) { if (NULL == ops || ops[i] > 3) return -1; cnt[ops[i]]++; }
        if (cnt[0] + cnt[1] + cnt[2] != rec->n || cnt[0] + cnt[1] + cnt[3] != rec->m) return -1;
    }
    if (0 != flappie_truth_write_fields(out, name, rec, ops, nops)) return -1;
    fprintf(out, "\t%s\t%c\t%ld\t%ld\n", ref->name[k], o, a, b);
    return 0;
}

void flappie_align_write_sam_header(FILE *out, const flappie_map_ref *ref) {
    fputs("@HD\tVN:1.6\tSO:unsorted\n", out);
    for (int k = 0; ref && k < ref->n; k++) fprintf(out, "@SQ\tSN:%s\tLN:%zu\n", ref->name[k], ref->len[k]);
    fputs("@PG\tID:flappie\n", out);
}

static void write_unmapped(FILE *out, const char *name, const char *seq, const char *qual, size_t n) {
    fprintf(out, "%s\t4\t*\t0\t0\t*\t*\t0\t0\t", name);
    if (0 == n) { fputs("*\t*\n", out); return; }
    for (size_t i = 0; i < n; i++) fputc('Z' == seq[i] ? 'C' : seq[i], out);
    fputc('\t', out);
    fwrite(qual, 1, n, out);
    fputc('\n', out);
}

int flappie_align_write_sam_line(FILE *out, const char *name, const char *seq, const char *qual, size_t n, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops,
                                 const ffhip_map_call *map, const flappie_map_ref *ref) {
    if (NULL == out || NULL == name || (n && (NULL == seq || NULL == qual))) return -1;
    if (NULL == rec || NULL == map || 1 != map->status || 1 != rec->status) { write_unmapped(out, name, seq, qual, n); return 0; }
    int k = 0;
    char o = '+';
    long a = 0, b = 0;
    if (NULL == ref || 0 != flappie_map_forward(ref, map->q, map->tstart, map->tend, &k, &o, &a, &b)) return -1;
    size_t cnt[4] = { 0, 0, 0, 0 };
    for (size_t i = 0; i < nops; i++) { if (NULL == ops || ops[i] > 3) return -1; cnt[ops[i]]++; }
    if (0 == n || cnt[0] + cnt[1] + cnt[2] != n || cnt[0] + cnt[1] + cnt[3] != (size_t)(b - a) || rec->n != n || (size_t)rec->dist != cnt[1] + cnt[2] + cnt[3]) return -1;
    const int rev = '-' == o;
    uint8_t *fops = rev ? malloc(nops ? nops : 1) : NULL;      /* the path from the forward strand's first base */
    if (rev && NULL == fops) return -1;
    for (size_t i = 0; rev && i < nops; i++) fops[i] = ops[nops - 1 - i];
    fprintf(out, "%s\t%d\t%s\t%ld\t255\t", name, rev ? 16 : 0, ref->name[k], a + 1);
    flappie_truth_write_cigar(out, rev ? fops : ops, nops);
    free(fops);
    fputs("\t*\t0\t0\t", out);
    for (size_t i = 0; i < n; i++) {
        const char c = seq[rev ? n - 1 - i : i], u = 'Z' == c ? 'C' : c;
        const char *at = strchr("ACGT", u);
        fputc(rev && at && u ? "TGCA"[at - "ACGT"] : u, out);
    }
    fputc('\t', out);
    for (size_t i = 0; i < n; i++) fputc(qual[rev ? n - 1 - i : i], out);
    fprintf(out, "\tNM:i:%d\n", rec->dist);
    return 1;
}

/*  flappie_output.c -- record formatting (include/flappie_output.h), byte-compatible with
 *  /root/reference/src/flappie_output.c:16-132 (including the SAM record's repeated sequence/quality
 *  line, which the reference emits); the records with SAMv1 1.7 base-modification tags
 *  (include/flappie_modbase.h); the records with the move table and signal tags (include/flappie_moves.h); and the records with
 *  the barcode tags behind any of those (include/flappie_barcodes.h); and the records with the adapter tags behind all of them, trimmed or split
 *  (include/flappie_adapters.h); and the records with the poly tail tags behind everything (include/flappie_polytail.h).
 */
#include <err.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/flappie_output.h"
#include "../../include/flappie_modbase.h"
#include "../../include/flappie_moves.h"
#include "../../include/flappie_barcodes.h"
#include "../../include/flappie_adapters.h"
#include "../../include/flappie_polytail.h"

enum flappie_outformat_type get_outformat(const char *formatstr) {
    if (NULL == formatstr) return FLAPPIE_OUTFORMAT_INVALID;
    if (0 == strcmp(formatstr, "fasta")) return FLAPPIE_OUTFORMAT_FASTA;
    if (0 == strcmp(formatstr, "fastq")) return FLAPPIE_OUTFORMAT_FASTQ;
    if (0 == strcmp(formatstr, "sam")) return FLAPPIE_OUTFORMAT_SAM;
    return FLAPPIE_OUTFORMAT_INVALID;
}

const char *flappie_outformat_string(enum flappie_outformat_type format) {
    switch (format) {
    case FLAPPIE_OUTFORMAT_FASTA: return "fasta";
    case FLAPPIE_OUTFORMAT_FASTQ: return "fastq";
    case FLAPPIE_OUTFORMAT_SAM: return "sam";
    case FLAPPIE_OUTFORMAT_INVALID: errx(EXIT_FAILURE, "Invalid flappie output %s:%d", __FILE__, __LINE__);
    default: errx(EXIT_FAILURE, "Flappie enum failure -- report bug\n");
    }
    return NULL;
}

static void put_string(FILE *fp, const char *str, bool newline) {
    if (NULL == fp || NULL == str) return;
    fputs(str, fp);
    if (newline) fputc('\n', fp);
}

/* flappie_output.c:95-100,112-117: the JSON-ish header shared by FASTA and FASTQ; `tail` goes in front of its newline ("" for the reference's records) */
static void put_header(FILE *fp, char lead, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                       const struct _raw_basecall_info *res, const char *tail) {
    fprintf(fp, "%c%s%s  { \"filename\" : \"%s\", \"uuid\" : \"%s\", \"normalised_score\" : %f,  \"nblock\" : %zu,  \"sequence_length\" : %zu,  \"blocks_per_base\" : %f, \"nsample\" : %zu, \"trim\" : [ %zu, %zu ] }%s\n",
            lead, prefix, uuid_primary ? uuid : readname, readname, uuid, -res->score / res->nblock, res->nblock,
            res->basecall_length, (float)res->nblock / (float)res->basecall_length, res->rt.n, res->rt.start, res->rt.end, tail);
}

void fprintf_fasta(FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                   const struct _raw_basecall_info res) {
    put_header(fp, '>', uuid, readname, uuid_primary, prefix, &res, "");
    put_string(fp, res.basecall, true);
    fflush(fp);
}

void fprintf_fastq(FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                   const struct _raw_basecall_info res) {
    if (NULL == res.quality) {
        warnx("Can't output fastq for reads without quality values");
        return;
    }
    put_header(fp, '@', uuid, readname, uuid_primary, prefix, &res, "");
    put_string(fp, res.basecall, true);
    fputs("+\n", fp);
    put_string(fp, res.quality, true);
    fflush(fp);
}

void fprintf_sam(FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                 const struct _raw_basecall_info res) {
    fprintf(fp, "%s%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n", prefix, uuid_primary ? uuid : readname, res.basecall,
            res.quality ? res.quality : "");
    put_string(fp, res.basecall, false);
    fputc('\t', fp);
    put_string(fp, res.quality, true);
    fflush(fp);
}

void fprintf_format(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname,
                    bool uuid_primary, const char *prefix, const struct _raw_basecall_info res) {
    switch (outformat) {
    case FLAPPIE_OUTFORMAT_FASTA: fprintf_fasta(fp, uuid, readname, uuid_primary, prefix, res); break;
    case FLAPPIE_OUTFORMAT_FASTQ: fprintf_fastq(fp, uuid, readname, uuid_primary, prefix, res); break;
    case FLAPPIE_OUTFORMAT_SAM: fprintf_sam(fp, uuid, readname, uuid_primary, prefix, res); break;
    case FLAPPIE_OUTFORMAT_INVALID: errx(EXIT_FAILURE, "Invalid flappie output %s:%d", __FILE__, __LINE__);
    default: errx(EXIT_FAILURE, "Flappie enum failure -- report bug\n");
    }
}

void printf_format(enum flappie_outformat_type outformat, const char *uuid, const char *readname, bool uuid_primary,
                   const char *prefix, const struct _raw_basecall_info res) {
    fprintf_format(outformat, stdout, uuid, readname, uuid_primary, prefix, res);
}

/* ---- records with base-modification tags (include/flappie_modbase.h) ---- */
int flappie_modbase_tags(const char *seq, const uint8_t *ml, char **mm_tag, char **ml_tag) {
    if (NULL == seq || NULL == mm_tag || NULL == ml_tag) return -1;
    *mm_tag = *ml_tag = NULL;
    size_t nc = 0;
    for (const char *c = seq; *c; c++) nc += ('C' == *c);
    if (nc > 0 && NULL == ml) return -1;
    char *mm = malloc(11 + 2 * nc + 1), *mv = malloc(7 + 4 * nc + 1);      /* "MM:Z:C+m?" ",0"... ";"  and  "ML:B:C" ",255"... */
    if (NULL == mm || NULL == mv) { free(mm); free(mv); return -1; }
    size_t a = 0, b = 0;
    memcpy(mm, "MM:Z:C+m?", 9); a = 9;
    memcpy(mv, "ML:B:C", 6); b = 6;
    for (size_t i = 0; seq[i]; i++) {      /* (digits by hand: a read has hundreds of Cs, and sprintf of each was most of the writer's time) */
        if ('C' != seq[i]) continue;
        mm[a++] = ','; mm[a++] = '0';
        const unsigned v = ml[i];
        mv[b++] = ',';
        if (v >= 100) mv[b++] = (char)('0' + v / 100);
        if (v >= 10) mv[b++] = (char)('0' + v / 10 % 10);
        mv[b++] = (char)('0' + v % 10);
    }
    mm[a++] = ';';
    mm[a] = 0;
    mv[b] = 0;
    *mm_tag = mm;
    *ml_tag = mv;
    return 0;
}

/* SEQ of a tagged record: the call with every Z written as C; and its two tags */
static char *modbase_seq(const struct _raw_basecall_info *res, const uint8_t *ml, char **mm, char **mv) {
    const char *call = res->basecall ? res->basecall : "";
    char *seq = strdup(call);
    if (NULL == seq) return NULL;
    for (char *c = seq; *c; c++) if ('Z' == *c) *c = 'C';
    if (0 != flappie_modbase_tags(seq, ml, mm, mv)) { free(seq); return NULL; }
    return seq;
}

/* a tagged record: SEQ and `tail` ("\t" + tags) in place of the call and of nothing -- FASTA / FASTQ with the tail in front of the header's newline, SAM as one line */
static void put_tagged_record(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                              const struct _raw_basecall_info *res, const char *seq, const char *tail) {
    switch (outformat) {
    case FLAPPIE_OUTFORMAT_FASTA:
        put_header(fp, '>', uuid, readname, uuid_primary, prefix, res, tail);
        put_string(fp, seq, true);
        break;
    case FLAPPIE_OUTFORMAT_FASTQ:
        put_header(fp, '@', uuid, readname, uuid_primary, prefix, res, tail);
        put_string(fp, seq, true);
        fputs("+\n", fp);
        put_string(fp, res->quality, true);
        break;
    case FLAPPIE_OUTFORMAT_SAM:      /* one line: the 11 mandatory fields, then the tags */
        fprintf(fp, "%s%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s%s\n", prefix, uuid_primary ? uuid : readname, seq, res->quality ? res->quality : "", tail);
        break;
    case FLAPPIE_OUTFORMAT_INVALID: errx(EXIT_FAILURE, "Invalid flappie output %s:%d", __FILE__, __LINE__);
    default: errx(EXIT_FAILURE, "Flappie enum failure -- report bug\n");
    }
    fflush(fp);
}

void fprintf_modbase_record(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname, bool uuid_primary,
                            const char *prefix, const struct _raw_basecall_info res, const uint8_t *ml) {
    if (FLAPPIE_OUTFORMAT_FASTQ == outformat && NULL == res.quality) {
        warnx("Can't output fastq for reads without quality values");
        return;
    }
    char *mm = NULL, *mv = NULL, *seq = modbase_seq(&res, ml, &mm, &mv);
    if (NULL == seq) errx(EXIT_FAILURE, "out of memory for the base-modification tags of %s", uuid_primary ? uuid : readname);
    char *tail = malloc(strlen(mm) + strlen(mv) + 3);
    if (NULL == tail) errx(EXIT_FAILURE, "out of memory for the base-modification tags of %s", uuid_primary ? uuid : readname);
    sprintf(tail, "\t%s\t%s", mm, mv);
    put_tagged_record(outformat, fp, uuid, readname, uuid_primary, prefix, &res, seq, tail);
    free(tail); free(seq); free(mm); free(mv);
}

/* ---- records with the move table and signal tags (include/flappie_moves.h) ---- */
double flappie_mean_quality(const char *quality) {
    if (NULL == quality || 0 == quality[0]) return 0.0;
    double perr[256], sum = 0.0;         /* 10^(-(Q - 33) / 10) of every character that occurs, computed once */
    bool have[256] = { false };
    size_t n = 0;
    for (const unsigned char *c = (const unsigned char *)quality; *c; c++, n++) {
        if (!have[*c]) { perr[*c] = pow(10.0, -((double)*c - 33.0) / 10.0); have[*c] = true; }
        sum += perr[*c];
    }
    return -10.0 * log10(sum / (double)n) + 0.0;      /* (+ 0.0: all '!' gives 0, not -0) */
}

static size_t put_uint(char *dst, size_t v) {
    char tmp[24];
    size_t k = 0, n;
    do { tmp[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    for (n = 0; n < k; n++) dst[n] = tmp[k - 1 - n];
    return k;
}

char *flappie_moves_tags(const uint8_t *moves, size_t nblock, int stride, const raw_table *rt, const char *quality, float median, float mad, bool delta) {
    if (NULL == rt || stride < 1 || stride > 127 || (nblock > 0 && NULL == moves)) return NULL;
    size_t b0 = 0;
    while (b0 < nblock && 0 == moves[b0]) b0++;         /* the first block with a move; nblock: an empty call */
    char *out = malloc(256 + 2 * (nblock - b0));
    if (NULL == out) return NULL;
    size_t a = 0;
    if (NULL != quality && 0 != quality[0]) a += (size_t)sprintf(out + a, "qs:f:%.3f\t", flappie_mean_quality(quality));
    memcpy(out + a, "ns:i:", 5); a += 5; a += put_uint(out + a, rt->n);
    memcpy(out + a, "\tts:i:", 6); a += 6; a += put_uint(out + a, rt->start + (size_t)stride * (b0 < nblock ? b0 : 0));
    if (!delta) a += (size_t)sprintf(out + a, "\tsm:f:%.9g\tsd:f:%.9g\tsv:Z:med_mad", (double)median, (double)mad);
    memcpy(out + a, "\tmv:B:c,", 8); a += 8; a += put_uint(out + a, (size_t)stride);
    for (size_t b = b0; b < nblock; b++) {              /* (digits by hand: a read has thousands of blocks) */
        out[a++] = ',';
        out[a++] = moves[b] ? '1' : '0';
    }
    out[a] = 0;
    return out;
}

void fprintf_moves_record(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                          const struct _raw_basecall_info res, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta) {
    if (FLAPPIE_OUTFORMAT_FASTQ == outformat && NULL == res.quality) {
        warnx("Can't output fastq for reads without quality values");
        return;
    }
    const char *name = uuid_primary ? uuid : readname;
    char *mm = NULL, *mv = NULL, *seq = NULL;
    if (NULL != ml) seq = modbase_seq(&res, ml, &mm, &mv);
    else seq = strdup(res.basecall ? res.basecall : "");
    char *tags = flappie_moves_tags(moves, res.nblock, stride, &res.rt, res.quality, median, mad, delta);
    if (NULL == seq || NULL == tags) errx(EXIT_FAILURE, "no move table tags for %s (out of memory, or a stride that does not fit int8)", name);
    char *tail = malloc((mm ? strlen(mm) + strlen(mv) + 2 : 0) + strlen(tags) + 2);
    if (NULL == tail) errx(EXIT_FAILURE, "out of memory for the move table tags of %s", name);
    if (mm) sprintf(tail, "\t%s\t%s\t%s", mm, mv, tags);
    else sprintf(tail, "\t%s", tags);
    put_tagged_record(outformat, fp, uuid, readname, uuid_primary, prefix, &res, seq, tail);
    free(tail); free(tags); free(seq); free(mm); free(mv);
}

/* ---- records with the barcode tags (include/flappie_barcodes.h): behind MM / ML and the move tags when the record carries those ---- */
void fprintf_barcode_record(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                            const struct _raw_basecall_info res, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta,
                            const ffhip_barcode_call *bc, const flappie_barcode_kit *kit, bool trim, bool reversed) {
    if (FLAPPIE_OUTFORMAT_FASTQ == outformat && NULL == res.quality) {
        warnx("Can't output fastq for reads without quality values");
        return;
    }
    const char *name = uuid_primary ? uuid : readname;
    if (trim && (NULL != ml || NULL != moves)) errx(EXIT_FAILURE, "barcodes are not trimmed from a record with base-modification or move tags (%s)", name);
    char *mm = NULL, *mv = NULL, *seq = NULL, *mtags = NULL, *qual = NULL;
    if (NULL != ml) seq = modbase_seq(&res, ml, &mm, &mv);
    else seq = strdup(res.basecall ? res.basecall : "");
    if (NULL != moves) mtags = flappie_moves_tags(moves, res.nblock, stride, &res.rt, res.quality, median, mad, delta);
    char *btags = flappie_barcode_tags(bc, kit);
    if (NULL == seq || NULL == btags || (NULL != moves && NULL == mtags)) errx(EXIT_FAILURE, "no barcode tags for %s (out of memory, or a record that does not belong to the kit)", name);
    struct _raw_basecall_info out = res;
    if (trim) {      /* the cuts are the call's in signal order; a reversed SEQ loses them at its other ends */
        const size_t len = strlen(seq);
        size_t from = 0, to = len;
        if (flappie_barcode_trim(bc, len, &from, &to)) warnx("%s: the barcode cuts at the two ends meet or cross; the record is written empty", name);
        else if (reversed) { const size_t f = len - to; to = len - from; from = f; }
        memmove(seq, seq + from, to - from);
        seq[to - from] = 0;
        if (NULL != res.quality && strlen(res.quality) == len && NULL != (qual = strndup(res.quality + from, to - from))) out.quality = qual;
    }
    char *tail = malloc((mm ? strlen(mm) + strlen(mv) + 2 : 0) + (mtags ? strlen(mtags) + 1 : 0) + strlen(btags) + 2);
    if (NULL == tail) errx(EXIT_FAILURE, "out of memory for the barcode tags of %s", name);
    size_t a = 0;
    if (mm) a += (size_t)sprintf(tail + a, "\t%s\t%s", mm, mv);
    if (mtags) a += (size_t)sprintf(tail + a, "\t%s", mtags);
    sprintf(tail + a, "\t%s", btags);
    put_tagged_record(outformat, fp, uuid, readname, uuid_primary, prefix, &out, seq, tail);
    free(tail); free(btags); free(mtags); free(seq); free(mm); free(mv); free(qual);
}

/* ---- records with the adapter tags (include/flappie_adapters.h): behind MM / ML, the move tags and the barcode tags when the record carries those; and with
 * `extra` (tags, no tab in front) behind them.  ad == NULL: no adapter tags, no adapter trim, no split ---- */
static void put_cut_record(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                           const struct _raw_basecall_info res, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta,
                           const ffhip_barcode_call *bc, const flappie_barcode_kit *bkit, bool bc_trim, const flappie_adapter_out *ad, bool reversed,
                           unsigned long long stats[4], const char *extra) {
    if (FLAPPIE_OUTFORMAT_FASTQ == outformat && NULL == res.quality) {
        warnx("Can't output fastq for reads without quality values");
        return;
    }
    const char *name = uuid_primary ? uuid : readname;
    const bool ad_trim = NULL != ad && ad->trim, ad_split = NULL != ad && ad->split;
    const bool cuts = bc_trim || ad_trim || ad_split;
    if (cuts && (NULL != ml || NULL != moves)) errx(EXIT_FAILURE, "adapters are not trimmed from a record with base-modification or move tags, nor is it split (%s)", name);
    char *mm = NULL, *mv = NULL, *seq = NULL, *mtags = NULL, *btags = NULL;
    if (NULL != ml) seq = modbase_seq(&res, ml, &mm, &mv);
    else seq = strdup(res.basecall ? res.basecall : "");
    if (NULL != moves) mtags = flappie_moves_tags(moves, res.nblock, stride, &res.rt, res.quality, median, mad, delta);
    if (NULL != bc) btags = flappie_barcode_tags(bc, bkit);
    char *atags = ad ? flappie_adapter_tags(ad->head, ad->hits, ad->kit) : NULL;
    if (NULL == seq || (NULL != ad && NULL == atags) || (NULL != bc && NULL == btags) || (NULL != moves && NULL == mtags))
        errx(EXIT_FAILURE, "no adapter tags for %s (out of memory, or a record that does not belong to the kit)", name);
    const size_t len = strlen(seq);
    /* the pieces to write, in signal order: the whole call, what the trims leave of it, or the pieces of a split read */
    flappie_adapter_piece pieces[FLAPPIE_ADAPTER_MAX_PIECES] = { { 0, len } };
    int npiece = 1, mode = FLAPPIE_SPLIT_WHOLE;
    size_t bfrom = 0, bto = len;
    int crossed = 0;
    if (bc_trim && NULL != bc) crossed = flappie_barcode_trim(bc, len, &bfrom, &bto);
    if (ad_split && !crossed) {
        int ndropped = 0;
        mode = flappie_adapter_split(ad->head, ad->hits, len, ad->window, ad->min_length, bfrom, bto, pieces, &npiece, &ndropped);
        if (FLAPPIE_SPLIT_OVERFLOW == mode) {
            if (stats) stats[3]++;
            warnx("%s: more than %d adapter hits; the read is not split", name, FFHIP_ADAPTER_MAX_HITS);
        } else if (FLAPPIE_SPLIT_SPLIT == mode && stats) { stats[0]++; stats[1] += (unsigned long long)npiece; stats[2] += (unsigned long long)ndropped; }
        else if (FLAPPIE_SPLIT_WHOLE == mode && 0 == pieces[0].to && len > 0) crossed = 1;
    }
    if (!ad_split || FLAPPIE_SPLIT_OVERFLOW == mode) {      /* one record: the larger cut at each end wins */
        size_t from = 0, to = len;
        npiece = 1;
        if (ad_trim && !crossed) crossed = flappie_adapter_trim(ad->head, ad->hits, len, ad->window, &from, &to);
        if (!crossed) {
            if (bfrom > from) from = bfrom;
            if (bto < to) to = bto;
            if (from >= to && len > 0) crossed = 1;
        }
        pieces[0].from = crossed ? 0 : from;
        pieces[0].to = crossed ? 0 : to;
    }
    if (crossed) {
        warnx("%s: the cuts at the two ends meet or cross; the record is written empty", name);
        pieces[0].from = pieces[0].to = 0;
        npiece = 1;
    }
    const size_t fixed = (mm ? strlen(mm) + strlen(mv) + 2 : 0) + (mtags ? strlen(mtags) + 1 : 0) + (btags ? strlen(btags) + 1 : 0) + (atags ? strlen(atags) + 1 : 0) + (extra ? strlen(extra) + 1 : 0) + 2;
    const bool named = FLAPPIE_SPLIT_SPLIT == mode;
    for (int k = 0; k < npiece; k++) {
        const size_t from = reversed ? len - pieces[k].to : pieces[k].from, to = reversed ? len - pieces[k].from : pieces[k].to;      /* a reversed SEQ holds the piece at its other end */
        struct _raw_basecall_info out = res;
        char *pseq = strndup(seq + from, to - from), *qual = NULL, *pname = NULL;
        char *tail = malloc(fixed + strlen(name) + 96);
        if (NULL == pseq || NULL == tail) errx(EXIT_FAILURE, "out of memory for the adapter tags of %s", name);
        if (NULL != res.quality && strlen(res.quality) == len && NULL != (qual = strndup(res.quality + from, to - from))) out.quality = qual;
        size_t a = 0;
        if (mm) a += (size_t)sprintf(tail + a, "\t%s\t%s", mm, mv);
        if (mtags) a += (size_t)sprintf(tail + a, "\t%s", mtags);
        if (btags) a += (size_t)sprintf(tail + a, "\t%s", btags);
        tail[a] = 0;
        if (atags) a += (size_t)sprintf(tail + a, "\t%s", atags);
        if (extra) a += (size_t)sprintf(tail + a, "\t%s", extra);
        if (named) {
            sprintf(tail + a, "\tpi:Z:%s\tsp:B:i,%zu,%zu", name, pieces[k].from, pieces[k].to);
            if (NULL == (pname = malloc(strlen(name) + 16))) errx(EXIT_FAILURE, "out of memory for the adapter tags of %s", name);
            sprintf(pname, "%s:%d", name, k + 1);
        }
        put_tagged_record(outformat, fp, (named && uuid_primary) ? pname : uuid, (named && !uuid_primary) ? pname : readname, uuid_primary, prefix, &out, pseq, tail);
        free(tail); free(pseq); free(qual); free(pname);
    }
    free(atags); free(btags); free(mtags); free(seq); free(mm); free(mv);
}

void fprintf_adapter_record(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                            const struct _raw_basecall_info res, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta,
                            const ffhip_barcode_call *bc, const flappie_barcode_kit *bkit, bool bc_trim, const flappie_adapter_out *ad, bool reversed,
                            unsigned long long stats[4]) {
    if (NULL == ad) errx(EXIT_FAILURE, "no adapter record for %s", uuid_primary ? uuid : readname);
    put_cut_record(outformat, fp, uuid, readname, uuid_primary, prefix, res, ml, moves, stride, median, mad, delta, bc, bkit, bc_trim, ad, reversed, stats, NULL);
}

/* ---- records with the poly tail tags (include/flappie_polytail.h): behind every other tag ---- */
void fprintf_polytail_record(enum flappie_outformat_type outformat, FILE *fp, const char *uuid, const char *readname, bool uuid_primary, const char *prefix,
                             const struct _raw_basecall_info res, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta,
                             const ffhip_barcode_call *bc, const flappie_barcode_kit *bkit, bool bc_trim, const flappie_adapter_out *ad, bool reversed,
                             unsigned long long stats[4], const ffhip_polytail *pt) {
    char *tags = flappie_polytail_tags(pt, res.rt.start);
    if (NULL == tags) errx(EXIT_FAILURE, "no poly tail tags for %s (out of memory, or no record)", uuid_primary ? uuid : readname);
    put_cut_record(outformat, fp, uuid, readname, uuid_primary, prefix, res, ml, moves, stride, median, mad, delta, bc, bkit, bc_trim, ad, reversed, stats, tags);
    free(tags);
}

/*  flappie_polytail.h -- the poly(A) tail of every read (flappie --poly-tail): options, tags, summary.
 *
 *  The tail itself is found on the GPU (FFHIP_RUN_POLYTAIL, include/ffhip.h "poly tail": the windows, the flags, the candidates, the record and the rate); this
 *  header is the host side: the options and their ranges, the tags of a record, the summary.
 *  The tags of a record, in this order and tab-separated, behind every other tag the record carries:
 *    status 1:       pt:i:  the tail's bases, rounded half away from zero
 *                    pa:B:i,<start>,<end>   the tail's samples [start, end) of the RAW signal (trim_start + first, trim_start + first + count)
 *                    pr:f:  samples a base of the rest of the read, as %.9g
 *    status 2 or 3:  pt:i:-1 alone (no tail found; a tail, but too few bases beside it to say how fast the read moves)
 *  Positions are raw samples of the signal, whatever --reverse, --trim-barcodes or --trim-adapters do to SEQ and QUAL.
 */
#ifndef FFHIP_FLAPPIE_POLYTAIL_H
#define FFHIP_FLAPPIE_POLYTAIL_H
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_adapters.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the --poly-tail-* options say: min_calls < 0 is "half the window, rounded up"; search is in SAMPLES. */
typedef struct {
    int base, from_end, window, min_calls, gap, min_windows;
    long search;
    int min_bases;
    float max_sd;
} flappie_polytail_opts;

/* A 8 blocks, half of them called, sd 0.3, gap 2, 5 windows, 20000 samples from the start, 20 bases */
void flappie_polytail_defaults(flappie_polytail_opts *o);
/* One option: `name` is the option's name behind "--poly-tail-" (base, window, min-calls, max-sd, gap, min-windows, search, min-bases), `value` its text.
 * 0, or -1 with the reason in err: a letter that is not one of ACGT, text that is not a number, a value outside the option's range. */
int flappie_polytail_set(flappie_polytail_opts *o, const char *name, const char *value, char *err, size_t errlen);
/* The kernel's parameters at a model's stride: min_calls' default, R = max(1, floor(search / (window stride))).  0, or -1 with the reason in err
 * (min_calls beyond the window). */
int flappie_polytail_params(const flappie_polytail_opts *o, int stride, ffhip_polytail_params *out, char *err, size_t errlen);

/* pt:i of a record: bases rounded half away from zero; -1 unless status is 1 */
long flappie_polytail_bases(const ffhip_polytail *rec);
/* The tags as one malloc'd string, no tab in front; NULL on a NULL record or when memory runs out. */
char *flappie_polytail_tags(const ffhip_polytail *rec, size_t trim_start);

/* The summary: reads with a record, with status 1, with status 3; the bases of the status 1 records. */
typedef struct { unsigned long long reads, found, no_rate; float *bases; size_t n, cap; } flappie_polytail_summary;
int flappie_polytail_count(flappie_polytail_summary *s, const ffhip_polytail *rec);        /* 0, or -1 when memory runs out */
double flappie_polytail_median(const flappie_polytail_summary *s);                          /* of bases over status 1 (an even count: the mean of the middle two); NAN of none */
/* polytail<TAB>reads|found|no_rate<TAB>count and polytail<TAB>median<TAB>%.1f */
void flappie_polytail_summary_print(FILE *fp, const flappie_polytail_summary *s);
void flappie_polytail_summary_free(flappie_polytail_summary *s);

/* One read with the poly tail tags last: what fprintf_adapter_record writes (ad == NULL: no adapter tags, bc == NULL: no barcode tags; ml, moves NULL: none of
 * theirs), and `pt` behind it. */
void fprintf_polytail_record(enum flappie_outformat_type fmt, FILE *out, const char *uuid, const char *filename, bool uuid_first, const char *prefix,
                             const flappie_call_t call, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta,
                             const ffhip_barcode_call *bc, const flappie_barcode_kit *bkit, bool bc_trim, const flappie_adapter_out *ad, bool reversed,
                             unsigned long long stats[4], const ffhip_polytail *pt);

#ifdef __cplusplus
}
#endif
#endif

/*  flappie_barcodes.h -- demultiplexing: which sample a read belongs to (flappie --barcodes kit.fa).
 *
 *  The kit is a FASTA file: a record's name (the header up to the first blank) is the barcode's name, its sequence -- on one line or several, in either
 *  case -- the pattern.  1 .. 128 records, patterns of 1 .. 128 bases over ACGT, every name once; anything else is refused.
 *  The classification itself is made on the GPU (FFHIP_RUN_BARCODES, include/ffhip.h "barcodes": the definitions of the windows, the infix edit distance
 *  and the rule); this header is the host side: the kit's parser, the tags of a record and the trim.
 *  The tags of a record, in this order and tab-separated, behind MM / ML and the move tags when the record carries those:
 *    BC:Z:  the barcode's name, or "unclassified"
 *    bd:i:  best_dist, the distance of the best barcode      bn:i:  second_dist, the runner-up's (255: a kit of one)
 *    bp:B:s,<front_end>,<rear_end>   where the best barcode's match ends at the front of the call and at the front of its reverse complement
 *  The tags always describe the call in SIGNAL order, whatever --reverse does to SEQ and QUAL.
 */
#ifndef FFHIP_FLAPPIE_BARCODES_H
#define FFHIP_FLAPPIE_BARCODES_H
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_output.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLAPPIE_BARCODE_MAX_KIT 128
#define FLAPPIE_BARCODE_MAX_LEN 128

typedef struct {
    int n;               /* records */
    char **name, **seq;  /* n strings each; the patterns in upper case */
    int lmin;            /* the shortest pattern: the default max_dist is lmin / 4 */
} flappie_barcode_kit;

/* The kit of a FASTA text / file.  NULL on a refusal (empty, more than 128 records, a pattern of more than 128 bases or of none, a character that is not
 * one of ACGT, a name twice or none, text in front of the first header; a file that cannot be read), with the reason in err. */
flappie_barcode_kit *flappie_barcode_kit_parse(const char *text, char *err, size_t errlen);
flappie_barcode_kit *flappie_barcode_kit_read(const char *path, char *err, size_t errlen);
void flappie_barcode_kit_free(flappie_barcode_kit *kit);

/* The four tags above as one malloc'd string, no tab in front; NULL on bad arguments (call->best beyond the kit) or when memory runs out. */
char *flappie_barcode_tags(const ffhip_barcode_call *call, const flappie_barcode_kit *kit);

/* --trim-barcodes: [*from, *to) of a call of `length` bases in signal order that stays -- a classified read (best >= 0) loses s[:front_end] when bit 0 of
 * `ends` is set and its last rear_end bases when bit 1 is; every other read stays whole.  Returns 1 when the two cuts meet or cross (*from = *to = 0:
 * the record is written empty), else 0. */
int flappie_barcode_trim(const ffhip_barcode_call *call, size_t length, size_t *from, size_t *to);

/* One record with the barcode tags: `call` as fprintf_format takes it (after any --reverse: `reversed` says so).  ml != NULL: MM / ML in front, as
 * fprintf_modbase_record writes them; moves != NULL: the move tags of fprintf_moves_record (stride, median, mad, delta are theirs) behind those; the barcode
 * tags come last.  trim: SEQ and QUAL are cut as flappie_barcode_trim says (ml and moves must be NULL then), nothing else of the record changes; a read
 * whose cuts cross is written with empty SEQ and QUAL and a warning. */
void fprintf_barcode_record(enum flappie_outformat_type fmt, FILE *out, const char *uuid, const char *filename, bool uuid_first, const char *prefix,
                            const flappie_call_t call, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta,
                            const ffhip_barcode_call *bc, const flappie_barcode_kit *kit, bool trim, bool reversed);

#ifdef __cplusplus
}
#endif
#endif

/*  flappie_adapters.h -- adapters and primers anywhere in a call (flappie --adapters kit.fa): tags, trimming, read splitting.
 *
 *  The kit is a FASTA file: a record's name (the header up to the first blank) is the adapter's name, its sequence -- on one line or several, in either
 *  case -- the pattern.  1 .. 32 records, patterns of 1 .. 64 bases over ACGT, every name once and without ',' or ';'; anything else is refused.
 *  The search itself is made on the GPU (FFHIP_RUN_ADAPTERS, include/ffhip.h "adapters": the definitions of the score rows, the hit rule, the start and the
 *  record); this header is the host side: the kit's parser, the tags of a record, the trim and the split.
 *  The tags of a record, in this order and tab-separated, behind MM / ML, the move tags and the barcode tags when the record carries those:
 *    an:i:  nhit, ALL hits of the read
 *    ah:Z:  <name>,<+|->,<start>,<end>,<dist>;  for each of the kept hits (at most 15, ordered by end): the hit covers s[start : end] of the call
 *  and, on the pieces of a split read (--split-reads):
 *    pi:Z:  the name of the read the piece was cut from        sp:B:i,<start>,<end>   the piece is s[start : end] of that read's call
 *  The tags always describe the call in SIGNAL order, whatever --reverse does to SEQ and QUAL.
 */
#ifndef FFHIP_FLAPPIE_ADAPTERS_H
#define FFHIP_FLAPPIE_ADAPTERS_H
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_barcodes.h"
#include "flappie_output.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLAPPIE_ADAPTER_MAX_KIT 32
#define FLAPPIE_ADAPTER_MAX_LEN 64
#define FLAPPIE_ADAPTER_MAX_PIECES (FFHIP_ADAPTER_MAX_HITS + 1)

typedef struct {
    int n;               /* records */
    char **name, **seq;  /* n strings each; the patterns in upper case */
} flappie_adapter_kit;

/* The kit of a FASTA text / file.  NULL on a refusal (empty, more than 32 records, a pattern of more than 64 bases or of none, a character that is not one
 * of ACGT, a name twice, none, or with ',' or ';', text in front of the first header; a file that cannot be read), with the reason in err. */
flappie_adapter_kit *flappie_adapter_kit_parse(const char *text, char *err, size_t errlen);
flappie_adapter_kit *flappie_adapter_kit_read(const char *path, char *err, size_t errlen);
void flappie_adapter_kit_free(flappie_adapter_kit *kit);

/* The two tags an / ah as one malloc'd string, no tab in front; NULL on bad arguments (kept beyond 15, a pattern beyond the kit) or when memory runs out. */
char *flappie_adapter_tags(const ffhip_adapter_header *head, const ffhip_adapter_hit *hits, const flappie_adapter_kit *kit);

/* --trim-adapters at window W: [*from, *to) of a call of `length` bases in signal order that stays.  The front cut is the largest `end` among the kept hits
 * with end <= W, the rear cut the smallest `start` among those with start >= length - W.  Returns 1 when the two cuts meet or cross (*from = *to = 0: the
 * record is written empty), else 0. */
int flappie_adapter_trim(const ffhip_adapter_header *head, const ffhip_adapter_hit *hits, size_t length, int window, size_t *from, size_t *to);

/* --split-reads at window W and least length M, within [clip_from, clip_to) of the call (0 and length: the whole call; the range --trim-barcodes keeps).
 * Returns the mode:
 *   FLAPPIE_SPLIT_OVERFLOW  nhit > 15: the record does not hold every hit, the read is written unsplit (*npiece = 0);
 *   FLAPPIE_SPLIT_WHOLE     no interior hit -- every kept hit is a front one (end <= W) or a rear one (start >= length - W): one piece, the range
 *                           flappie_adapter_trim keeps within the clip, whatever its length (from = to = 0 when the cuts cross), written under the read's own name;
 *   FLAPPIE_SPLIT_SPLIT     the pieces are the maximal stretches of that range covered by no kept hit, in signal order; those shorter than M are dropped and
 *                           counted in *ndropped.  *npiece may be 0. */
enum { FLAPPIE_SPLIT_WHOLE = 0, FLAPPIE_SPLIT_SPLIT = 1, FLAPPIE_SPLIT_OVERFLOW = 2 };
typedef struct { size_t from, to; } flappie_adapter_piece;
int flappie_adapter_split(const ffhip_adapter_header *head, const ffhip_adapter_hit *hits, size_t length, int window, size_t min_length, size_t clip_from, size_t clip_to,
                          flappie_adapter_piece pieces[FLAPPIE_ADAPTER_MAX_PIECES], int *npiece, int *ndropped);

/* What --adapters asks of a record: the read's record and the kit; trim / split with their parameters. */
typedef struct {
    const ffhip_adapter_header *head;
    const ffhip_adapter_hit *hits;
    const flappie_adapter_kit *kit;
    bool trim, split;
    int window;
    size_t min_length;
} flappie_adapter_out;

/* One read with the adapter tags, as fprintf_barcode_record writes it (bc == NULL: no barcode tags; bc_trim as its `trim`), the adapter tags last.
 * ad->trim: SEQ and QUAL are cut as flappie_adapter_trim says; with bc_trim too, the larger cut at each end wins.  ad->split: as flappie_adapter_split
 * says -- a split read becomes one record a piece, named <name>:<k>, k = 1 ... over the pieces written, each with pi and sp behind the adapter tags, and
 * --reverse reverses each piece as it would the whole call; an overflowing read is written as without ad->split.  ml and moves must be NULL with any of the
 * three.  stats[4] are counted up: reads split, pieces written, pieces dropped, reads that overflowed. */
void fprintf_adapter_record(enum flappie_outformat_type fmt, FILE *out, const char *uuid, const char *filename, bool uuid_first, const char *prefix,
                            const flappie_call_t call, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta,
                            const ffhip_barcode_call *bc, const flappie_barcode_kit *bkit, bool bc_trim, const flappie_adapter_out *ad, bool reversed,
                            unsigned long long stats[4]);

#ifdef __cplusplus
}
#endif
#endif

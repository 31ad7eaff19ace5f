/*  flappie_remap.h -- the host side of flappie --remap refs.fa --remap-out map.tsv: each read's signal mapped to a sequence the user knows.
 *
 *  The mapping itself is made on the GPU (FFHIP_RUN_REMAP, include/ffhip.h "remap": the flip-flop coding, the band, the recursion and its tie rule); this
 *  header is the reader of the sequences, the derivation of start[] and maxdev from a read's moves, and the line of map.tsv.
 *  refs.fa is a FASTA file: a record's name runs up to the first blank of its header, its sequence stands on one line or several, lower case is upper-cased.
 *  A record with a letter outside the model's alphabet (ACGT, or ACGTZ) is kept as BAD: its read gets status 2, as does one with more bases than blocks + 1
 *  and one whose scores leave no finite path (include/ffhip.h "remap").  A read finds its record by its read id
 *  first, then by its file's base name (with or without the extension).  Sequences are in SIGNAL order.
 *  map.tsv, one line per read that had a record, tab-separated:
 *    name  status  nblock  stride  trim_start  L  band  maxdev  score(%.9g)  start[0],start[1],...     (maxdev, score and start[] are * for status 2)
 *  With --remap-from-map (a line per read the map placed, the sequence its stretch of the reference) four columns follow: record  strand  tstart  tend, as in hits.tsv.
 *  Base i starts at block start[i] (start[0] = 0, start[i] = 1 + the index of the i-th one of the moves), block b stands for samples
 *  [trim_start + b stride, ...); maxdev = max_b |p_b - c(b)| says whether the band was touched (maxdev = band).
 */
#ifndef FFHIP_FLAPPIE_REMAP_H
#define FFHIP_FLAPPIE_REMAP_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the largest --remap-band: the widest kernel form holds a window of 4608 cells (include/ffhip.h "remap"), and a window is at most 2 W + 1.  A wider band would
 * make a whole batch fail for one long sequence, so the option is refused instead. */
#define FLAPPIE_REMAP_BAND_MAX 2303

typedef struct {
    int n;               /* records */
    char **name;         /* n names */
    uint8_t **codes;     /* n sequences as codes 0 .. strlen(alphabet) - 1 (NULL for a bad record) */
    size_t *len;         /* their lengths */
    int *bad;            /* 1: the record holds a letter outside the alphabet */
    int *order;          /* the records' indices sorted by name (the first of equal names first) */
} flappie_remap_refs;

/* The records of a FASTA text / file over `alphabet` ("ACGT" or "ACGTZ").  NULL with the reason in err: no text, text in front of the first header, a header
 * without a name, a file that cannot be read, no memory.  An empty file gives n = 0. */
flappie_remap_refs *flappie_remap_refs_parse(const char *text, const char *alphabet, char *err, size_t errlen);
flappie_remap_refs *flappie_remap_refs_read(const char *path, const char *alphabet, char *err, size_t errlen);
void flappie_remap_refs_free(flappie_remap_refs *refs);
/* the record of a read: by its read id, then by its file's base name, then by that without its extension; -1: none */
int flappie_remap_refs_find(const flappie_remap_refs *refs, const char *read_id, const char *filename);
/* start[0 .. L - 1] and maxdev of nblock moves that sum to L - 1; -1 (nothing written) when they do not, or L = 0 */
int flappie_remap_starts(const uint8_t *rm, size_t nblock, size_t L, size_t *start, size_t *maxdev);
/* one line of map.tsv; rm may be NULL unless status is 1.  Returns maxdev (0 for the other statuses), -1 on moves that do not fit L */
long flappie_remap_write_line(FILE *out, const char *name, int status, size_t nblock, int stride, size_t trim_start, size_t L, int band, const uint8_t *rm, float score);
/* flappie --remap-from-map: the same line with the read's place behind it, as hits.tsv and acc.tsv have it: the record's name, the strand (+ or -) and the span
 * [tstart, tend) on the record's forward strand.  The sequence is the mapped stretch in signal order, L = tend - tstart.  Same return; -1 too (nothing written) for
 * a NULL argument, another strand or a span that is none */
long flappie_remap_write_placed_line(FILE *out, const char *name, int status, size_t nblock, int stride, size_t trim_start, size_t L, int band, const uint8_t *rm, float score,
                                     const char *record, char strand, long tstart, long tend);

#ifdef __cplusplus
}
#endif
#endif

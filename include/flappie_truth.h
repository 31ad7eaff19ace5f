/*  flappie_truth.h -- the host side of flappie --truth refs.fa --truth-out acc.tsv: each read's call scored against the sequence it should have been.
 *
 *  The alignment itself is made on the GPU (FFHIP_RUN_TRUTH, include/ffhip.h "truth": the band, the recursion, the traceback's rule); this header is the line of
 *  acc.tsv, with the ops run-length coded as an extended CIGAR (=XID), and the summary.  refs.fa is read and searched by flappie_remap_refs_read and
 *  flappie_remap_refs_find (include/flappie_remap.h): one record a read, by read id, then by file name, in SIGNAL order.
 *  acc.tsv, one line per read that had a record, tab-separated:
 *    name  status  n  m  band  maxdev  dist  matches  mismatches  insertions  deletions  identity(%.6f)  CIGAR       (maxdev .. CIGAR are * unless status is 1)
 *  identity = matches / (matches + mismatches + insertions + deletions); the CIGAR reads the path from the first base: = match, X mismatch, I a called base the
 *  truth lacks, D a base of the truth the call lacks.  An alignment without ops (n = m = 0 cannot be: m >= 1) has no line of its own form.
 */
#ifndef FFHIP_FLAPPIE_TRUTH_H
#define FFHIP_FLAPPIE_TRUTH_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the largest --truth-band: the widest kernel form holds a window of 2560 cells (include/ffhip.h "truth"), and a window is at most 2 W + 1 */
#define FLAPPIE_TRUTH_BAND_MAX 1279
#define FLAPPIE_TRUTH_BAND_DEFAULT 512

typedef struct {
    int status;                          /* 1 aligned, 2 not aligned (an empty or refused record, or a band that leaves no path) */
    size_t n, m;                         /* called bases, bases of the truth */
    int band, maxdev, dist, n_match, n_mismatch, n_ins, n_del;
} flappie_truth_rec;

typedef struct {
    unsigned long long aligned, not_aligned, no_record, band_touched;
    unsigned long long matches, columns; /* pooled over the aligned reads: identity = matches / columns */
    double *identity;                    /* the aligned reads' identities (owned) */
    size_t nid, cap;
} flappie_truth_summary;

/* matches / (matches + mismatches + insertions + deletions); 0 for an alignment of no columns */
double flappie_truth_identity(const flappie_truth_rec *rec);
/* the CIGAR of nops ops (0 '=', 1 'X', 2 'I', 3 'D') written to `out`; "*" for none.  Returns the characters written, -1 for an op > 3 */
long flappie_truth_write_cigar(FILE *out, const uint8_t *ops, size_t nops);
/* one line of acc.tsv; ops may be NULL unless status is 1.  Returns 0, -1 for ops that do not fit the record's counts (nothing is written then) */
int flappie_truth_write_line(FILE *out, const char *name, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops);
/* the same thirteen columns without the end of the line, for a table that puts columns of its own behind them (include/flappie_align.h) */
int flappie_truth_write_fields(FILE *out, const char *name, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops);
/* the summary: a read with a record (rec != NULL) or without one; 0, -1 when memory runs out */
int flappie_truth_summary_add(flappie_truth_summary *sum, const flappie_truth_rec *rec);
double flappie_truth_summary_pooled(const flappie_truth_summary *sum);
/* the median of the aligned reads' identities (the mean of the middle two for an even count; 0 for none); sorts the list */
double flappie_truth_summary_median(flappie_truth_summary *sum);
/* "truth\taligned\t..." lines: aligned, not_aligned, no_record, band_touched, pooled_identity, median_identity */
void flappie_truth_summary_print(FILE *out, flappie_truth_summary *sum);
void flappie_truth_summary_free(flappie_truth_summary *sum);

#ifdef __cplusplus
}
#endif
#endif

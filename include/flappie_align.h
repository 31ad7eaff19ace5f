/*  flappie_align.h -- the host side of flappie --map ref.fa --truth-from-map --truth-out acc.tsv [--map-sam aln.sam]: each call aligned to the stretch of the
 *  reference it was mapped to, in the run that mapped it.
 *
 *  Map and alignment are made on the GPU (FFHIP_RUN_MAP | FFHIP_RUN_TRUTH after ffhip_batch_set_truth_from_map, include/ffhip.h "truth from map"); this header is
 *  the line of acc.tsv in that mode and the aligned SAM file.
 *  acc.tsv, one line per read whose map status is 1, tab-separated: the thirteen columns of include/flappie_truth.h with the read's name as in hits.tsv, then
 *    record  strand  tstart  tend            (forward strand, half open: hits.tsv's values for that read)
 *  The CIGAR of acc.tsv stays in SIGNAL order, as under --truth.
 *  aln.sam: "@HD VN:1.6 SO:unsorted", one "@SQ SN:<name> LN:<length>" a record of the reference in file order (a name runs to the first white space),
 *  "@PG ID:flappie", then one line per read with a call, in output order.  A read whose map status and truth status are both 1:
 *    name  FLAG (0, or 16 for the - strand)  RNAME  POS = forward tstart + 1  MAPQ 255  CIGAR  *  0  0  SEQ  QUAL  NM:i:<dist>
 *  with everything in FORWARD-strand order: the ops run-length coded with =XID and reversed for the - strand, SEQ the whole call with Z written as C and
 *  reverse-complemented for the - strand, QUAL reversed for the - strand.  Every other read with a call: name  4  *  0  0  *  *  0  0  SEQ  QUAL  (signal order).
 *  `seq` and `qual` are always the whole call in signal order.
 */
#ifndef FFHIP_FLAPPIE_ALIGN_H
#define FFHIP_FLAPPIE_ALIGN_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_map.h"
#include "flappie_truth.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one line of acc.tsv in the mode; `map` has status 1.  Returns 0, -1 (nothing written) for ops that do not fit the record's counts or a map record that does not
 * fit the reference */
int flappie_align_write_acc_line(FILE *out, const char *name, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops, const ffhip_map_call *map,
                                 const flappie_map_ref *ref);
/* the header lines of aln.sam */
void flappie_align_write_sam_header(FILE *out, const flappie_map_ref *ref);
/* one line of aln.sam: seq and qual are the call's n letters in signal order; rec, ops and map may be NULL for a read without them (written unmapped).  Returns 1
 * for an aligned line, 0 for an unmapped one, -1 (nothing written) for a map record that does not fit the reference, ops that do not fit the call and the span, or
 * no memory */
int flappie_align_write_sam_line(FILE *out, const char *name, const char *seq, const char *qual, size_t n, const flappie_truth_rec *rec, const uint8_t *ops, size_t nops,
                                 const ffhip_map_call *map, const flappie_map_ref *ref);

#ifdef __cplusplus
}
#endif
#endif

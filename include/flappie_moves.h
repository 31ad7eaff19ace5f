/*  flappie_moves.h -- records that say where in the signal each called base sits: the move table and signal tags that guppy
 *  (--moves_out) and dorado (--emit-moves) write and remora, f5c, uncalled4 and squigualiser read (flappie --emit-moves).
 *
 *  A read of nblock blocks has one move byte a block (FFHIP_RUN_MOVES, include/ffhip.h): move[b] = 1 where block b's transition emits a
 *  base, and block b stands for the samples [rt.start + b * stride, rt.start + (b + 1) * stride) of the raw signal, clipped to rt.end.
 *  The tags of a record, in this order and tab-separated:
 *    qs:f:  mean quality of the call, -10 log10( mean_i 10^(-(Q_i - 33) / 10) ), %.3f; absent for an empty call
 *    ns:i:  rt.n, the samples in the file
 *    ts:i:  rt.start + stride * b0, b0 the first block with a move (an empty call: rt.start)
 *    sm:f: sd:f: sv:Z:med_mad   the median and the MAD (x 1.4826) the read was normalised with, %.9g: (pA - sm) / sd is the signal the
 *           network saw; all three absent under --delta
 *    mv:B:c,  the stride, then move[b0 .. nblock - 1] as 0 / 1 (starts with a 1, ends with a 0; an empty call: the stride alone)
 *  mv is in SIGNAL order whatever the orientation of SEQ: with --reverse (RNA) SEQ, QUAL and ML are reversed and mv is not, as in
 *  dorado's RNA records.
 */
#ifndef FFHIP_FLAPPIE_MOVES_H
#define FFHIP_FLAPPIE_MOVES_H
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include "flappie_output.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Mean quality of a quality string (the qs tag's value), in double; a NULL or empty string: 0 */
double flappie_mean_quality(const char *quality);

/* The tags above as one malloc'd string, tab-separated, no tab in front: moves is nblock bytes (may be NULL when nblock is 0), stride in 1 .. 127,
 * rt gives n and start, quality the call's quality string (NULL or "": no qs), median / mad the normalisation, delta whether the read was prepared
 * with --delta (no sm / sd / sv).  Returns NULL on bad arguments or when memory runs out; the caller frees the string. */
char *flappie_moves_tags(const uint8_t *moves, size_t nblock, int stride, const raw_table *rt, const char *quality, float median, float mad, bool delta);

/* One record with the tags: `call` as fprintf_format takes it (after any --reverse; call.nblock is the length of moves), moves in signal order.
 * ml == NULL: SEQ is the call as it is; otherwise the record carries MM / ML in front of these tags as fprintf_modbase_record writes them (ml aligned
 * with call.basecall, Z written as C).
 *   FASTA / FASTQ: fprintf_fasta / fprintf_fastq's bytes with "\t" + tags in front of the header's newline;
 *   SAM: ONE line, QNAME 4 * 0 0 * * 0 0 SEQ QUAL and the tags. */
void fprintf_moves_record(enum flappie_outformat_type fmt, FILE *out, const char *uuid, const char *filename, bool uuid_first, const char *prefix,
                          const flappie_call_t call, const uint8_t *ml, const uint8_t *moves, int stride, float median, float mad, bool delta);

#ifdef __cplusplus
}
#endif
#endif

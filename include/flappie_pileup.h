/*  flappie_pileup.h -- the host side of flappie --map ref.fa --truth-from-map --map-pileup pileup.tsv [--map-pileup-min-identity N]: per position of the
 *  reference, how many aligned calls cover it and what they say there.
 *
 *  The counters are made on the GPU (FFHIP_RUN_PILEUP into one ffhip_pileup for the whole run, include/ffhip.h "pileup") and come down once, at the end; this
 *  header is the table and the summary.
 *  pileup.tsv, no header, one line for every position of every record in reference order, sixteen tab-separated columns:
 *    record  position (0-based)  reference letter  depth  A+ C+ G+ T+ del+ ins+  A- C- G- T- del- ins-
 *  depth = the ten counts of A, C, G, T and del on both strands; an insertion stands at the position to its LEFT on the forward strand; the base counts of the -
 *  strand are of the forward strand's letters (the call reverse-complemented).  Inserted letters are not kept.
 *  stderr: "pileup<TAB>key<TAB>integer" for reads, skipped, positions, covered (depth >= 1), match, mismatch, del, ins, edge_ins.
 */
#ifndef FFHIP_FLAPPIE_PILEUP_H
#define FFHIP_FLAPPIE_PILEUP_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the table from the downloaded planes (counts: [12][P], P the reference's bases together); *covered, when given, takes the positions of depth >= 1.
 * Returns 0, -1 for a NULL argument */
int flappie_pileup_write(FILE *out, const flappie_map_ref *ref, const uint32_t *counts, unsigned long long *covered);
/* the lines of stderr */
void flappie_pileup_summary_print(FILE *out, const ffhip_pileup_totals *totals, unsigned long long positions, unsigned long long covered);

#ifdef __cplusplus
}
#endif
#endif

/*  flappie_consensus.h -- the host side of flappie --map ref.fa --truth-from-map --map-consensus cons.fa [--map-consensus-changes changes.tsv]
 *  [--map-consensus-min-depth N] [--map-consensus-min-identity N]: the sample's sequence per record of the reference, and where it differs from the reference.
 *
 *  The counters are made on the GPU (FFHIP_RUN_CONSENSUS into one ffhip_consensus for the whole run, include/ffhip.h "consensus"), the cells are called there too
 *  (ffhip_consensus_call) and both come down once, at the end; this header is the two files and the summary.
 *  cons.fa: one FASTA record per record of the reference, in reference order: ">name", then the letters of the record's cells concatenated, in lines of 70.  A
 *    position below the depth writes the reference's letter in lower case; a record whose consensus is empty writes its header and an empty line.
 *  changes.tsv, no header, one line for every cell that is not plain SAME or LOW (a substitution, a deletion, or any cell with inserted letters), seven
 *    tab-separated columns:
 *    record  position (0-based)  reference letter  the cell's letters ("-" if none)  depth  the winner's count  the first insertion column's total (0 if none)
 *  stderr: "consensus<TAB>key<TAB>integer" for reads, skipped, positions, called (depth >= min depth), low_depth, same, sub, del, ins (the inserted letters
 *    written), long_ins, edge_ins.
 */
#ifndef FFHIP_FLAPPIE_CONSENSUS_H
#define FFHIP_FLAPPIE_CONSENSUS_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_map.h"

#ifdef __cplusplus
extern "C" {
#endif

/* what the cells say, counted by flappie_consensus_write: same, sub and del are the called positions by their winner; ins the inserted letters written */
typedef struct { unsigned long long positions, called, low_depth, same, sub, del, ins; } flappie_consensus_stats;

/* cons.fa from the called cells (cells: [P], P the reference's bases together); *stats, when given, takes the counts.  Returns 0, -1 for a NULL argument */
int flappie_consensus_write(FILE *out, const flappie_map_ref *ref, const ffhip_consensus_cell *cells, flappie_consensus_stats *stats);
/* changes.tsv from the cells and the downloaded planes (counts: [37][P]).  Returns 0, -1 for a NULL argument */
int flappie_consensus_changes_write(FILE *out, const flappie_map_ref *ref, const ffhip_consensus_cell *cells, const uint32_t *counts);
/* the lines of stderr */
void flappie_consensus_summary_print(FILE *out, const ffhip_consensus_totals *totals, const flappie_consensus_stats *stats);

#ifdef __cplusplus
}
#endif
#endif

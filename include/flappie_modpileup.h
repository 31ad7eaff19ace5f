/*  flappie_modpileup.h -- the host side of flappie --map ref.fa --truth-from-map --map-mods mods.bed [--map-mods-hi N] [--map-mods-lo N] [--map-mods-min-identity N]
 *  [--map-mods-motif CG|C] [--map-mods-combine-strands] [--map-mods-hist hist.tsv]: per C of the reference, how methylated the aligned calls say it is.
 *
 *  The counters are made on the GPU (FFHIP_RUN_MOD_PILEUP into one ffhip_modpileup for the whole run, include/ffhip.h "mod pileup") and come down once, at the end;
 *  this header is the table, the histogram's file and the summary.
 *  mods.bed, no header, bedMethyl as `modkit pileup` writes it: one row for (record k, forward position f, strand o) when
 *    the position is a site of that strand (the record's letter at f, upper-cased as --map does: C for +, G for -);
 *    it passes the motif -- C: every site; CG: + needs G at f + 1, - needs C at f - 1, and a record's ends have no neighbour;
 *    its five counters sum to 1 or more.
 *  Rows in reference order, + before - at one position.  Eighteen tab-separated columns:
 *    record  f  f+1  m  Nvalid  strand  f  f+1  255,0,0  Nvalid  percent  mod  canon  0  del  fail  diff  0
 *  Nvalid = mod + canon; percent = "%.2f" of 100.0 * mod / Nvalid, "0.00" when Nvalid is 0.
 *  combine (CG only): the - strand's counters of the G at f + 1 are added to the + strand's row of the C at f; strand '.', no - row.
 *  hist.tsv: 256 lines "byte<TAB>count".
 *  stderr: "mods_pileup<TAB>key<TAB>integer" for reads, skipped, sites, mod, canon, fail, diff, del, rows (the lines written).
 */
#ifndef FFHIP_FLAPPIE_MODPILEUP_H
#define FFHIP_FLAPPIE_MODPILEUP_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_map.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { FLAPPIE_MODS_MOTIF_CG = 0, FLAPPIE_MODS_MOTIF_C = 1 };

/* the table from the downloaded planes (counts: [10][P], P the reference's bases together); *rows, when given, takes the lines written.
 * Returns 0, -1 for a NULL argument, a motif that is neither, or combine with another motif than CG */
int flappie_modpileup_write(FILE *out, const flappie_map_ref *ref, const uint32_t *counts, int motif, int combine, unsigned long long *rows);
/* hist.tsv from the downloaded histogram (256 words) */
int flappie_modpileup_hist_write(FILE *out, const uint64_t *hist);
/* the lines of stderr */
void flappie_modpileup_summary_print(FILE *out, const ffhip_modpileup_totals *totals, unsigned long long rows);

#ifdef __cplusplus
}
#endif
#endif

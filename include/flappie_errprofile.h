/*  flappie_errprofile.h -- the host side of flappie --truth refs.fa | --map ref.fa --truth-from-map, --truth-out acc.tsv --truth-errors errors.tsv
 *  [--truth-errors-min-identity N]: the run's error profile -- which truth base is called as which, what the qualities are worth, which 5-mers go wrong and how
 *  homopolymers come out.
 *
 *  The counters are made on the GPU (FFHIP_RUN_ERRPROFILE into one ffhip_errprofile for the whole run, include/ffhip.h "error profile") and come down once, at the
 *  end; this header is the table and the summary.
 *  errors.tsv, no header, tab-separated, integers only:
 *    sub   truth letter  called letter (A C G T, - a deletion)  count                    all 20 lines
 *    ins   inserted letter  count                                                       4 lines
 *    qual  q (0 .. 93)  matches  mismatches  inserted letters                            all 94 lines
 *    ctx   the truth's 5-mer  match  mismatch  del at its centre  ins behind its centre  the 5-mers with a count, in order of w
 *    hp    the run's letter  its true length r (1 .. 16)  its called length c  count     the cells with a count, in order; c = 32 means 32 or more
 *  A counter is written as it stands, up to 2^64 - 1.
 *  stderr: "errors<TAB>key<TAB>integer" for reads, skipped, match, mismatch, del, ins, edge_ins, ctx_sites, hp_runs, hp_long, hp_wide, reserved.
 */
#ifndef FFHIP_FLAPPIE_ERRPROFILE_H
#define FFHIP_FLAPPIE_ERRPROFILE_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the table from the downloaded counters (counts: [FFHIP_ERRPROFILE_TABLE_WORDS]).  Returns 0, -1 for a NULL argument */
int flappie_errprofile_write(FILE *out, const uint64_t *counts);
/* the lines of stderr */
void flappie_errprofile_summary_print(FILE *out, const ffhip_errprofile_totals *totals);

#ifdef __cplusplus
}
#endif
#endif

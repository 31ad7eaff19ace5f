/*  flappie_sitemods.h -- the host side of flappie --remap ... --remap-mods mods.tsv: the scores at every C of a mapped sequence.
 *
 *  The scores are made on the GPU (FFHIP_RUN_REMAP_MODS, include/ffhip.h "site mods": the sites, the window, the two hypotheses and the recursion); this header is
 *  the line of mods.tsv.  One line per site, tab-separated, no header:
 *    name  pos  letter (the given one: C or Z)  nblock  can(%.9g)  mod(%.9g)  can - mod(%.9g, the difference taken in double)
 *  No exp is taken here: p(5mC) = 1 / (1 + exp(can - mod)) is the reader's, and the file does not depend on a libm.
 */
#ifndef FFHIP_FLAPPIE_SITEMODS_H
#define FFHIP_FLAPPIE_SITEMODS_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a mapped read's lines: its nsm records in the order given; codes: the L codes of its sequence in `alphabet`.  Returns 0, or -1 (nothing more is written) at a
 * record whose pos lies outside the sequence or whose letter there is neither C nor Z. */
int flappie_sitemods_write(FILE *out, const char *name, const uint8_t *codes, size_t L, const char *alphabet, const ffhip_site_mod *sm, size_t nsm);

#ifdef __cplusplus
}
#endif
#endif

/*  flappie_variants.h -- the host side of flappie --remap ... --remap-variants vars.tsv --remap-variants-out calls.tsv: ref against alt alleles of mapped reads.
 *
 *  The scores are made on the GPU (FFHIP_RUN_REMAP_VARIANTS, include/ffhip.h "variants": the window, the two hypotheses and the recursion); this header is the
 *  reader of vars.tsv and the line of calls.tsv.
 *  vars.tsv, one variant a line, tab-separated:  name  pos  ref  alt
 *    name  a record of --remap's file, looked up as a read looks its record up (exactly, then as a file's base name, then without its extension);
 *    pos   0-based in that record, in signal order;
 *    ref, alt  letters of the model's alphabet (lower case is upper-cased), at most 16 each; `-` stands for an empty allele.  ref must be the record's
 *          letters at pos: `A 7 - G` inserts G in front of position 7 (pos = the record's length: behind its last base), `A 7 CG -` deletes positions 7 and 8.
 *  Lines that start with `#` and empty lines are ignored.  A line that cannot be used is SKIPPED and counted by kind, never an error.
 *  calls.tsv, one line per variant of a mapped read, tab-separated, no header:
 *    name  pos  ref  alt  nblock  ref(%.9g)  alt(%.9g)  ref - alt(%.9g, the difference taken in double)
 *  -inf prints as printf gives it.  The difference is never nan: an alt score of -inf gives inf, two scores of -inf give 0.  No exp is taken here: the
 *  probability is the reader's, and the file does not depend on a libm.
 */
#ifndef FFHIP_FLAPPIE_VARIANTS_H
#define FFHIP_FLAPPIE_VARIANTS_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"
#include "flappie_remap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* why a line was skipped */
enum { FLAPPIE_VARIANTS_MALFORMED = 0,     /* not four fields, an empty field, pos not a whole number >= 0, both alleles empty, an edit that leaves no base */
       FLAPPIE_VARIANTS_LETTER,            /* a letter outside the alphabet */
       FLAPPIE_VARIANTS_LONG,              /* an allele longer than 16 */
       FLAPPIE_VARIANTS_NO_RECORD,         /* no record of that name, or one that holds a letter outside the alphabet */
       FLAPPIE_VARIANTS_BEYOND,            /* pos + the ref allele lies beyond the record */
       FLAPPIE_VARIANTS_REF_MISMATCH,      /* ref is not the record's letters at pos */
       FLAPPIE_VARIANTS_KINDS };

typedef struct {
    size_t n;                                               /* variants kept, in file order */
    int *rec;                                               /* n: the record of the sequences each belongs to */
    ffhip_variant *var;                                     /* n */
    int nrec;                                               /* the records of the sequences */
    size_t *first;                                          /* nrec + 1: a record's entries of idx */
    size_t *idx;                                            /* n: the variants grouped by record, in file order within a record */
    unsigned long long skipped[FLAPPIE_VARIANTS_KINDS];     /* lines skipped, by kind */
    size_t skipped_line[FLAPPIE_VARIANTS_KINDS];            /* the first of each kind: its line number from 1 (0: none) ... */
    char skipped_text[FLAPPIE_VARIANTS_KINDS][128];         /* ... and its text, cut at 127 bytes */
} flappie_variants;

/* what a kind is called in a message */
const char *flappie_variants_kind(int kind);
/* The variants of a text / file against the records `refs` over `alphabet` ("ACGT" or "ACGTZ").  NULL with the reason in err: no text, no records, a file that
 * cannot be read, no memory.  An empty file gives n = 0. */
flappie_variants *flappie_variants_parse(const char *text, const flappie_remap_refs *refs, const char *alphabet, char *err, size_t errlen);
flappie_variants *flappie_variants_read(const char *path, const flappie_remap_refs *refs, const char *alphabet, char *err, size_t errlen);
void flappie_variants_free(flappie_variants *vs);
/* the variants of record `rec` in file order: their number, and (out given) a copy of them */
size_t flappie_variants_of(const flappie_variants *vs, int rec, ffhip_variant *out);
/* a mapped read's lines: its n variants and their records, vc[i].index naming the variant; codes: the L codes of its sequence in `alphabet`.  Returns 0, or -1
 * (nothing more is written) at a record whose index is not below n or whose variant does not fit the sequence. */
int flappie_variants_write(FILE *out, const char *name, const uint8_t *codes, size_t L, const char *alphabet, const ffhip_variant *var, const ffhip_variant_call *vc, size_t n);

#ifdef __cplusplus
}
#endif
#endif

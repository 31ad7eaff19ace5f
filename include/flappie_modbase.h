/*  flappie_modbase.h -- records of a model with a modified base (r941_5mC) carrying the SAMv1 1.7 base-modification tags
 *  MM / ML instead of the letter Z in the sequence (flappie --modbase-tags).
 *
 *  SEQ is the called string with every Z written as C; MM:Z:C+m? lists every C of SEQ (all skip counts 0), ML:B:C gives each
 *  of them its byte N, the probability of 5mC in [N/256, (N+1)/256) (FFHIP_RUN_MOD_PROBS, include/ffhip.h).
 */
#ifndef FFHIP_FLAPPIE_MODBASE_H
#define FFHIP_FLAPPIE_MODBASE_H
#include <stdbool.h>
#include <stdint.h>
#include <stdio.h>
#include "flappie_output.h"
#include "networks.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 when the registry's model calls a modified base (a 5-base alphabet with Z), else 0 */
int flappie_model_has_modbase(enum model_type model);

/* The two tags of one record: seq is SEQ as written (no Z), ml one byte per base of seq (only those at a C are read; may be NULL when seq has no C).
 * *mm_tag = "MM:Z:C+m?" + ",0" per C + ";",  *ml_tag = "ML:B:C" + ",N" per C -- malloc'd, the caller frees them.  Returns 0, or -1 (bad arguments, no memory). */
int flappie_modbase_tags(const char *seq, const uint8_t *ml, char **mm_tag, char **ml_tag);

/* One record with the tags: `call` as fprintf_format takes it (the basecall with its Zs, after any --reverse) and ml aligned with call.basecall.
 *   FASTA / FASTQ: fprintf_fasta / fprintf_fastq's bytes with "\tMM:Z:...\tML:B:C..." in front of the header's newline, SEQ in place of the call;
 *   SAM: ONE line, QNAME 4 * 0 0 * * 0 0 SEQ QUAL MM ML (fprintf_sam's repeated sequence / quality line is not written). */
void fprintf_modbase_record(enum flappie_outformat_type fmt, FILE *out, const char *uuid, const char *filename, bool uuid_first, const char *prefix,
                            const flappie_call_t call, const uint8_t *ml);

#ifdef __cplusplus
}
#endif
#endif

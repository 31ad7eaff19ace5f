/*  flappie_map.h -- the host side of flappie --map ref.fa --map-out hits.tsv: each read's call placed on a small reference (the lambda control, a plasmid, a
 *  mitochondrion, a virus, an amplicon panel), on either strand.
 *
 *  The search itself is made on the GPU (FFHIP_RUN_MAP, include/ffhip.h "map": the anchors, the score rows, the best place and its tie rule, the start, the bound,
 *  the pairing rule); this header is the reader of the reference, the turn from a strand's coordinates to the forward strand's, the line of hits.tsv, the record of
 *  --map-records, and the summary.
 *  ref.fa is a FASTA file: a record's name runs up to the first blank of its header, its sequence stands on one line or several, lower case (soft-masked) letters
 *  are upper-cased.  Refused, each with a text: an empty file, a record without a sequence, a name that occurs twice, more than 1024 records, more than 2^20 bases
 *  together, and any letter that is not one of ACGT (N and the IUPAC codes are not guessed) -- with the record and the position.
 *  hits.tsv, one line per read in output order, no header, tab-separated:
 *    name  status  n  anchors  record  strand  tstart  tend  length  front_dist  front_second  rear_dist  rear_second
 *  status: 0 no call, 1 mapped, 2 unmapped (an anchor over its bound), 3 discordant (the anchors disagree).  record, strand (+ or -), tstart, tend (forward strand,
 *  half open) and the record's length are * unless status is 1.  For status 2 and 3 eight further columns say where each anchor went on its own:
 *    front_record  front_strand  front_start  front_end  rear_record  rear_strand  rear_start  rear_end      (forward strand)
 *  --map-records recs.fa: for every mapped read ">name" and y_q[tstart : tend] -- the read's own stretch of the reference in SIGNAL order, reverse-complemented for
 *  the - strand: the file --remap takes (in a second run: its sequences are set before a batch runs), and --truth too, which --truth-from-map spares
 *  (include/flappie_align.h).
 *  A search's coordinates [start, end) in y_q are [start, end) on the forward strand for strand + and [m - end, m - start) for strand -.
 */
#ifndef FFHIP_FLAPPIE_MAP_H
#define FFHIP_FLAPPIE_MAP_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include "ffhip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FLAPPIE_MAP_MAX_RECORDS 1024
#define FLAPPIE_MAP_WINDOW_DEFAULT 4096
#define FLAPPIE_MAP_MAX_ERROR_DEFAULT 250

typedef struct {
    int n;               /* records */
    char **name;         /* n names */
    char **seq;          /* n sequences over ACGT, upper case */
    size_t *len;         /* their lengths */
} flappie_map_ref;

typedef struct { unsigned long long reads, mapped, unmapped, discordant, dist, bases; } flappie_map_summary;

/* The records of a FASTA text / file.  NULL with the reason in err. */
flappie_map_ref *flappie_map_ref_parse(const char *text, char *err, size_t errlen);
flappie_map_ref *flappie_map_ref_read(const char *path, char *err, size_t errlen);
void flappie_map_ref_free(flappie_map_ref *ref);
/* [start, end) of search q on the forward strand of its record: 0, or -1 (nothing written) for a q or a span the reference does not hold */
int flappie_map_forward(const flappie_map_ref *ref, int q, long start, long end, int *record, char *strand, long *fstart, long *fend);
/* one line of hits.tsv: 0, or -1 (nothing written) for a record that does not fit the reference */
int flappie_map_write_line(FILE *out, const char *name, const ffhip_map_call *rec, const flappie_map_ref *ref);
/* the read's own stretch as a FASTA record: 1 written, 0 not mapped (nothing written), -1 a record that does not fit the reference */
int flappie_map_write_record(FILE *out, const char *name, const ffhip_map_call *rec, const flappie_map_ref *ref);
/* the summary: a read's record, with the window its run had (<= 0: the default); "map\treads\t..." lines: reads, mapped, unmapped, discordant, anchor_dist,
 * anchor_bases and pooled_error = anchor_dist / anchor_bases over the anchors of the mapped reads (%.6f; 0 for none) */
void flappie_map_summary_add(flappie_map_summary *sum, const ffhip_map_call *rec, int window);
void flappie_map_summary_print(FILE *out, const flappie_map_summary *sum);

#ifdef __cplusplus
}
#endif
#endif

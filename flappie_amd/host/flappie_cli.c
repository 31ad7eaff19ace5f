/*  flappie -- command line of the MI355X flip-flop basecaller.
 *
 *  Same option table, defaults, file/directory globbing and per-read output as the reference's
 *  src/flappie.c (options :42-67, defaults :93-112, parse :127-239, main :319-399).  The body differs where
 *  it has to: the reference calls calculate_post() per file (flappie.c:371); here files are read and
 *  prepared on the host, grouped by trimmed length (the network never pads or splits a read) and sent to
 *  the HIP engine in batches; records are written in input order.
 */
#ifndef _GNU_SOURCE
#define _GNU_SOURCE      /* sched_setaffinity, CPU_SET (bind_to_gpu_numa) */
#endif
#include <sched.h>
#include <argp.h>
#include <assert.h>
#include <dirent.h>
#include <err.h>
#include <sys/stat.h>
#include <glob.h>
#include <libgen.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <pthread.h>
#include <semaphore.h>
#include <string.h>
#include <time.h>
#include <strings.h>
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>
#include <execinfo.h>

#include "../../include/decode.h"
#include "../../include/fast5_interface.h"
#include "../../include/ffhip.h"
#include "../../include/flappie_common.h"
#include "../../include/flappie_output.h"
#include "../../include/flappie_modbase.h"
#include "../../include/flappie_sitemods.h"
#include "../../include/flappie_variants.h"
#include "../../include/flappie_moves.h"
#include "../../include/flappie_barcodes.h"
#include "../../include/flappie_adapters.h"
#include "../../include/flappie_map.h"
#include "../../include/flappie_polytail.h"
#include "../../include/flappie_remap.h"
#include "../../include/flappie_truth.h"
#include "../../include/flappie_align.h"
#include "../../include/flappie_pileup.h"
#include "../../include/flappie_modpileup.h"
#include "../../include/flappie_consensus.h"
#include "../../include/flappie_errprofile.h"
#include "../../include/networks.h"

const char *argp_program_version = "flappie (MI355X/HIP) 0.1, interface of flappie 2.1.3";
const char *argp_program_bug_address = "<this repository>";
#ifdef BUILD_RUNNIE
static char doc[] = "Runnie basecaller -- basecall from raw signal";
#else
static char doc[] = "Flappie basecaller -- basecall from raw signal";
#endif
static char args_doc[] = "fast5 [fast5 ...]";
static struct argp_option options[] = {
    {"delta", 'd', "factor", 0, "Using delta samples model with scaling factor"},
    {"format", 'f', "format", 0, "Format to output reads (FASTA or SAM)"},
    {"limit", 'l', "nreads", 0, "Maximum number of reads to call (0 is unlimited)"},
    {"model", 'm', "name", 0, "Model to use (\"help\" to list)"},
    {"output", 'o', "filename", 0, "Write to file rather than stdout"},
    {"prefix", 'p', "string", 0, "Prefix to append to name of each read"},
#ifdef BUILD_RUNNIE
    {"reverse", 'r', 0, 0, "Reverse output base calls"},
#else
    {"reverse", 'r', 0, 0, "Reverse output base calls (the mv tag of --emit-moves and the barcode tags of --barcodes keep describing the call in signal order)"},
#endif
    {"no-reverse", 6, 0, OPTION_ALIAS, "Don't reverse output base calls"},
    {"temperature", 7, "factor", 0, "Temperature for weights"},
    {"trim", 't', "start:end", 0, "Number of samples to trim, as start:end"},
    {"trace", 'T', "filename", 0, "Dump trace to HDF5 file"},
    {"licence", 10, 0, 0, "Print licensing information"},
    {"license", 11, 0, OPTION_ALIAS, "Print licensing information"},
    {"segmentation", 3, "chunk:percentile", 0, "Chunk size and percentile for variance based segmentation"},
    {"viterbi", 'v', 0, 0, "Use viterbi decoding only"},
    {"no-viterbi", 8, 0, OPTION_ALIAS, "Use forward-backward followed by viterbi"},
    {"fb", 9, 0, OPTION_ALIAS, "Use forward-backward followed by viterbi"},
    {"hdf5-compression", 12, "level", 0, "Gzip compression level for HDF5 output (0:off, 1: quickest, 9: best)"},
    {"hdf5-chunk", 13, "size", 0, "Chunk size for HDF5 output"},
    {"uuid", 14, 0, 0, "Output UUID"},
    {"no-uuid", 15, 0, OPTION_ALIAS, "Output read file"},
    {"batch", 16, "nreads", 0, "Reads per GPU batch (default: what one layer launch takes -- 1024 at up to 256 hidden units, 512 up to 384, else 256)"},
    {"shard", 18, "g/n", 0, "Call only files g, g+n, g+2n, ... of the sorted input list (one process per GPU: tools/flappie_multi_gpu.sh)"},
    {"readers", 17, "n", 0, "fast5 reader processes feeding the GPU (default 4: one keeps up with ~50 Msamples/s of files that need libhdf5 and > 200 of those host/fast5_raw.c reads; more only cost CPU; 0 reads in this process)"},
    {"shard-by-size", 19, 0, 0, "With --shard: deal the files to the n shards by size (largest first, each to the lightest shard) instead of by index"},
#ifdef BUILD_RUNNIE
    {"fasta", 20, 0, 0, "Write FASTA basecalls instead of run records: what the run records through misc/decode_runnie.py give, with runs and run lengths made on the GPU"},
    {"rlc", 21, 0, 0, "With --fasta: the run-length compressed sequence (one base a run, as decode_runnie.py --rlc)"},
    {"run-scale", 22, "A,C,G,T", 0, "With --fasta: per-base factors of the scale parameter (default 1.02,1.04,1.04,1.02, as decode_runnie.py --scale)"},
#else
    {"modbase-tags", 23, 0, 0, "Report modified bases as SAM MM/ML tags (5mC probabilities made on the GPU): Z is written as C and every C gets a probability (models with a modified base only, e.g. r941_5mC)"},
    {"emit-moves", 24, 0, 0, "Report where in the signal each base sits: the move table and signal tags of guppy --moves_out / dorado --emit-moves (qs, ns, ts, sm, sd, sv, mv), with the moves made on the GPU. mv is always in signal order: with --reverse SEQ, QUAL and ML are reversed and mv is not"},
    {"barcodes", 25, "kit.fa", 0, "Demultiplex: classify every read against the barcodes of a FASTA file (1-128 records, the record's name is the barcode's, patterns of 1-128 bases over ACGT), scored on the GPU at both ends of the call. Every record gains BC:Z:<name> (or unclassified), bd:i: (best distance), bn:i: (runner-up's distance) and bp:B:s,<front_end>,<rear_end>, behind MM / ML and the move tags; a summary of reads per barcode goes to stderr. The tags describe the call in signal order, with --reverse too"},
    {"barcode-window", 26, "bases", 0, "With --barcodes: bases searched at each end of a call (1-256, default 150)"},
    {"barcode-max-dist", 27, "edits", 0, "With --barcodes: largest edit distance of an accepted barcode (default: a quarter of the kit's shortest pattern, rounded down)"},
    {"barcode-min-sep", 28, "edits", 0, "With --barcodes: least distance between the best barcode and the runner-up (default 3)"},
    {"barcode-both-ends", 29, 0, 0, "With --barcodes: a barcode must be found at both ends (its score is the larger of its two distances)"},
    {"trim-barcodes", 30, 0, 0, "With --barcodes: cut the barcode and what precedes it from SEQ and QUAL of classified reads, at each end where it was found (not with --emit-moves, --modbase-tags or --trace)"},
    {"adapters", 269, "kit.fa", 0, "Find sequencing adapters and primers anywhere in every call: the records of a FASTA file (1-32 records, the record's name is the adapter's, patterns of 1-64 bases over ACGT), every occurrence in both orientations with exact start and end, searched on the GPU. Every record gains an:i:<hits> and ah:Z:<name>,<+|->,<start>,<end>,<dist>;... (at most 15 hits, ordered by end), behind the barcode tags; a summary of hits per adapter goes to stderr. The tags describe the call in signal order, with --reverse too"},
    {"adapter-max-dist", 270, "edits", 0, "With --adapters: largest edit distance of a hit (default: a quarter of each pattern's length, rounded down)"},
    {"trim-adapters", 271, 0, 0, "With --adapters: cut SEQ and QUAL behind the last hit that ends within --adapter-window bases of the front, and in front of the first hit that starts within as many bases of the rear; with --trim-barcodes the larger cut at each end wins (not with --emit-moves, --modbase-tags or --trace)"},
    {"adapter-window", 272, "bases", 0, "With --trim-adapters or --split-reads: how far from an end of the call a hit is an end's adapter (default 150)"},
    {"split-reads", 273, 0, 0, "With --adapters: a read with a hit in its interior is two molecules called as one: write every stretch of the call that no hit covers as a record of its own, named <name>:<k> in signal order, with pi:Z:<name> and sp:B:i,<start>,<end>; a read without an interior hit is written whole, trimmed at its ends; a read with more than 15 hits is written unsplit (not with --emit-moves, --modbase-tags, --trace, --remap or --truth)"},
    {"split-min-length", 274, "bases", 0, "With --split-reads: pieces shorter than this are dropped and counted (default 200)"},
    {"poly-tail", 275, 0, 0, "Measure every read's poly(A) tail on the GPU: the stretch of signal that stays flat while the model says the tail's base, divided by the samples a base of the rest of the read. Every record gains pt:i:<bases>, pa:B:i,<start>,<end> (raw samples) and pr:f:<samples a base>, or pt:i:-1 where no tail or no rate was found, behind every other tag; a summary goes to stderr (not with --split-reads)"},
    {"poly-tail-base", 276, "letter", 0, "With --poly-tail: the tail's base, one of ACGT (default A)"},
    {"poly-tail-end", 277, 0, 0, "With --poly-tail: search from the signal's end, for cDNA reads whose tail is there"},
    {"poly-tail-window", 278, "blocks", 0, "With --poly-tail: blocks a window (1-64, default 8)"},
    {"poly-tail-min-calls", 279, "blocks", 0, "With --poly-tail: blocks of the tail's base a window needs (0 to the window; default half the window, rounded up)"},
    {"poly-tail-max-sd", 280, "sd", 0, "With --poly-tail: largest standard deviation of a flat window's samples, in the units of the normalised signal (default 0.3)"},
    {"poly-tail-gap", 281, "windows", 0, "With --poly-tail: windows that are not flat a tail may bridge (0-16, default 2)"},
    {"poly-tail-min-windows", 282, "windows", 0, "With --poly-tail: shortest tail kept (default 5)"},
    {"poly-tail-search", 283, "samples", 0, "With --poly-tail: how far from the chosen end of the signal a tail may begin (default 20000)"},
    {"poly-tail-min-bases", 284, "bases", 0, "With --poly-tail: called bases beside the tail that the rate needs (default 20)"},
    {"remap", 31, "refs.fa", 0, "Map each read's signal to a sequence you already know: the records of a FASTA file, found by read id, then by the file's base name, in SIGNAL order (reverse them yourself for --reverse and RNA). The best path of the read's transition scores through its sequence is made on the GPU and written to --remap-out; stdout does not change"},
    {"remap-out", 256, "map.tsv", 0, "With --remap: one line per read that had a record: name, status (1 mapped, 2 not: a letter outside the model's alphabet, or more bases than blocks + 1), nblock, stride, trim_start, L, band, maxdev, score and the block every base starts at"},
    {"remap-band", 257, "W", 0, "With --remap: the band's half-width in sequence positions around the straight line from (0, 0) to (nblock, L - 1) (0-2303, default 2048: the GPU holds a window of at most 2 W + 1 <= 4608 positions; maxdev = W in map.tsv says the band was touched)"},
    {"remap-events", 261, "events.tsv", 0, "With --remap: the signal under every base of every mapped read, made on the GPU from the mapping and the read's normalised signal: one line per base, reads in output order and bases in signal order, no header: name, base index, base letter, first raw sample, samples, mean and standard deviation (population form; a base without samples has 0 for both)"},
    {"remap-mods", 262, "mods.tsv", 0, "With --remap, a model with a modified base (r941_5mC): at every C or Z of every mapped read's sequence, the log scores of the signal around it with C and with 5mC at that position, made on the GPU from the mapping and the read's transition scores: one line per site, reads in output order and sites in signal order, no header: name, position, the given letter, blocks of the window, score with C, score with 5mC, and their difference (the log-likelihood ratio; p(5mC) = 1 / (1 + exp(ratio)))"},
    {"remap-mods-context", 263, "N", 0, "With --remap-mods: the bases either side of a site whose signal is scored (0-31, default 15)"},
    {"remap-mods-all-paths", 264, 0, 0, "With --remap-mods: sum over all paths of the window in double precision instead of taking the best path"},
    {"remap-variants", 265, "vars.tsv", 0, "With --remap: for every variant of a tab-separated file (name, pos, ref, alt: the record's name as --remap finds it, the 0-based position in the record in signal order, the record's letters there and the letters to put in their place, at most 16 each, - for none), the log scores of the signal around it under the record as given and as edited, made on the GPU from the mapping and the read's transition scores, written to --remap-variants-out; a line that cannot be used is skipped and counted"},
    {"remap-variants-out", 266, "calls.tsv", 0, "With --remap-variants (required): one line per variant of every mapped read, reads in output order and variants in file order, no header: name, pos, ref, alt, blocks of the window, score of ref, score of alt, and their difference (the log-likelihood ratio)"},
    {"remap-variants-context", 267, "N", 0, "With --remap-variants: the bases either side of an edit whose signal is scored (1-23, default 10)"},
    {"remap-variants-all-paths", 268, 0, 0, "With --remap-variants: sum over all paths of the window in double precision instead of taking the best path"},
    {"truth", 258, "refs.fa", 0, "Score each read's call against the sequence it should have been: the records of a FASTA file, found as for --remap (the same file may serve both), in SIGNAL order. The whole call is aligned to its record on the GPU (banded global edit distance) and the result written to --truth-out; stdout does not change. The alignment is always of the whole call in signal order: --reverse and --trim-barcodes do not alter it"},
    {"truth-out", 259, "acc.tsv", 0, "With --truth (required): one line per read that had a record: name, status (1 aligned, 2 not: an empty record, a letter outside the model's alphabet, or a band that leaves no path), n, m, band, maxdev, dist, matches, mismatches, insertions, deletions, identity and the extended CIGAR (=XID)"},
    {"truth-band", 260, "W", 0, "With --truth: the band's half-width in called bases around the straight line from (0, 0) to (m, n) (0-1279, default 512: the GPU holds a window of at most 2 W + 1 <= 2560 cells; maxdev = W in acc.tsv says the band was touched)"},
    {"map", 285, "ref.fa", 0, "Place every read's call on a small reference (the lambda control, a plasmid, a mitochondrion, a virus, an amplicon panel): the records of a FASTA file (1-1024 records over ACGT, at most 1048576 bases together; lower case is upper-cased, N and IUPAC letters are refused). The first and the last --map-window bases of the call are searched on both strands of every record on the GPU (infix edit distance) and the result written to --map-out; stdout does not change. The whole call is mapped in signal order: --reverse, --trim-barcodes, --trim-adapters and --split-reads do not alter it"},
    {"map-out", 286, "hits.tsv", 0, "With --map (required): one line per read, no header: name, status (0 no call, 1 mapped, 2 unmapped, 3 discordant), n, anchors, record, strand, tstart, tend (forward strand), the record's length, and distance and runner-up of the front and the rear anchor; for status 2 and 3 record, strand, start and end of either anchor behind them"},
    {"map-window", 287, "W", 0, "With --map: bases of an anchor (64-4096, default 4096); a call of more has two, its first and its last W bases"},
    {"map-max-error", 288, "permille", 0, "With --map: largest edit distance of an anchor, and largest difference between the span on the reference and the call's length, in thousandths of their lengths (0-500, default 250)"},
    {"map-records", 289, "recs.fa", 0, "With --map: for every mapped read a FASTA record of its own stretch of the reference in signal order (reverse-complemented for the - strand): the file --remap takes in a second run (--truth too, which --truth-from-map spares)"},
    {"truth-from-map", 290, 0, 0, "With --map and --truth-out: align every mapped read's call to its own stretch of the reference in the same run, on the GPU, as --truth would in a second run with the file of --map-records. acc.tsv gets one line per mapped read: the thirteen columns of --truth-out with the read's name as in hits.tsv, then record, strand, tstart and tend as in hits.tsv; the CIGAR stays in signal order. --truth-band applies; not with --truth. stdout, hits.tsv and recs.fa do not change"},
    {"remap-from-map", 307, 0, 0, "With --map and --remap-out: map every mapped read's signal to its own stretch of the reference in the same run, on the GPU, as --remap would in a second run with the file of --map-records. map.tsv gets one line per mapped read: the columns of --remap-out with the read's name as in hits.tsv, then record, strand, tstart and tend as in hits.tsv; the starts stay in signal order. --remap-band and --remap-events apply (a base's letter is the reference's, turned to the read's strand), and --truth-from-map goes in the same run; not with --remap, --remap-mods or --remap-variants. stdout, hits.tsv, acc.tsv and every other file do not change"},
    {"map-sam", 291, "aln.sam", 0, "With --truth-from-map: the alignments as a SAM file with @SQ lines: one line per read with a call, in output order; a read that is mapped and aligned with FLAG 0 or 16, POS, the CIGAR (=XID) in forward-strand order, SEQ (Z written as C) and QUAL turned to the forward strand and NM:i; every other read unmapped (FLAG 4). SEQ is always the whole call: --reverse, --trim-barcodes, --trim-adapters and --split-reads do not alter it"},
    {"map-pileup", 292, "pileup.tsv", 0, "With --truth-from-map: per position of the reference, the aligned calls' counts, added up on the GPU over the whole run and written at its end: one line for every position of every record in reference order, no header: record, 0-based position, reference letter, depth (A, C, G, T and del of both strands), then A, C, G, T, del, ins of the + strand and of the - strand. An insertion stands at the position to its left on the forward strand; insertions before the first or behind the last aligned base are counted on stderr only (edge_ins). Inserted letters are not kept. The whole call counts: --reverse, --trim-barcodes, --trim-adapters and --split-reads do not alter it. stdout, hits.tsv, acc.tsv and aln.sam do not change"},
    {"map-pileup-min-identity", 293, "permille", 0, "With --map-pileup: count only reads whose alignment's identity, matches over matches + mismatches + insertions + deletions, is at least this many thousandths (0-1000, default 0); the others are counted as skipped"},
    {"map-mods", 294, "mods.bed", 0, "With --truth-from-map and a model with a modified base (r941_5mC): per C of the reference, how methylated the aligned calls say it is, added up on the GPU over the whole run and written at its end as a bedMethyl table (the eighteen columns of modkit pileup, no header, modification code m): a row for every C of the + strand and every G of the - strand that passes --map-mods-motif and is covered. A C or Z call on such a site counts as modified when its 5mC byte (ML, floor(256 p)) is at least --map-mods-hi, as canonical when it is at most --map-mods-lo, and as failed between; another letter counts as Ndiff, a deletion as Ndelete. The 5mC bytes are made whether or not --modbase-tags is given. The whole call counts: --reverse, the trims and --split-reads do not alter it. stdout, hits.tsv, acc.tsv, aln.sam and pileup.tsv do not change"},
    {"map-mods-hi", 295, "byte", 0, "With --map-mods: a 5mC byte of at least this is a modified call (0-255, above --map-mods-lo; default 205, p >= 0.8). The default comes from reasoning, not from reads: see --map-mods-hist"},
    {"map-mods-lo", 296, "byte", 0, "With --map-mods: a 5mC byte of at most this is a canonical call (0-255, below --map-mods-hi; default 50, p < 0.2)"},
    {"map-mods-min-identity", 297, "permille", 0, "With --map-mods: count only reads whose alignment's identity is at least this many thousandths (0-1000, default 0), as --map-pileup-min-identity"},
    {"map-mods-motif", 298, "CG|C", 0, "With --map-mods: the sites written: CG (default: a C followed by a G, and on the - strand a G behind a C) or C (every C, every G on the - strand)"},
    {"map-mods-combine-strands", 299, 0, 0, "With --map-mods and the motif CG: one row a CpG, the - strand's counts of its G added to the + strand's row of its C, strand '.'"},
    {"map-mods-hist", 300, "hist.tsv", 0, "With --map-mods: 256 lines of byte and count: how many counted C or Z calls on a site had each 5mC byte -- the distribution to choose --map-mods-hi and --map-mods-lo from"},
    {"map-consensus", 301, "cons.fa", 0, "With --truth-from-map: the sample's sequence per record of the reference, from the aligned calls' bases, deletions and inserted letters, counted on the GPU over the whole run and called there at its end: one FASTA record per record of the reference, in reference order, in lines of 70. Per position the most frequent of A, C, G, T and deletion is written (a tie goes to the reference's letter, else to the first in that order), then up to 8 inserted letters behind it, each while more than half of the position's depth has one. A position below --map-consensus-min-depth writes the reference's letter in lower case. Letters of an insertion beyond the eighth are counted on stderr only (long_ins), as are insertions before the first or behind the last aligned base (edge_ins). No polishing round, no qualities. The whole call counts: --reverse, the trims and --split-reads do not alter it. stdout, hits.tsv, acc.tsv, aln.sam, pileup.tsv and mods.bed do not change"},
    {"map-consensus-changes", 302, "changes.tsv", 0, "With --map-consensus: where the consensus differs from the reference: one line for every position with a substitution, a deletion or inserted letters, no header: record, 0-based position, reference letter, the letters written there (- if none), depth, the winner's count, the first inserted letter's count (0 if none)"},
    {"map-consensus-min-depth", 303, "N", 0, "With --map-consensus: a position covered by fewer aligned calls than this keeps the reference's letter, in lower case (1-65535, default 3). The default comes from reasoning, not from reads"},
    {"map-consensus-min-identity", 304, "permille", 0, "With --map-consensus: count only reads whose alignment's identity is at least this many thousandths (0-1000, default 0), as --map-pileup-min-identity"},
    {"truth-errors", 305, "errors.tsv", 0, "With --truth and --truth-out, or with --truth-from-map: the run's error profile, counted on the GPU over all the aligned reads and written once at the end, no header, integers only: 20 lines 'sub', truth letter, called letter (- a deletion), count; 4 lines 'ins', inserted letter, count; 94 lines 'qual', quality, matches, mismatches, inserted letters with it; 'ctx', the truth's 5-mer, matches, mismatches and deletions at its centre and insertions behind it, for every 5-mer with a count; 'hp', letter, true length (1-16), called length (32: 32 or more), count, for every homopolymer run inside a truth. Runs longer than 16 and runs whose alignment takes more than 64 ops are counted on stderr only (hp_long, hp_wide), as are insertions before the first or behind the last truth base (edge_ins). The whole call counts: --reverse, the trims and --split-reads do not alter it. stdout, acc.tsv, hits.tsv and every other file do not change"},
    {"truth-errors-min-identity", 306, "permille", 0, "With --truth-errors: count only reads whose alignment's identity is at least this many thousandths (0-1000, default 0), as --map-pileup-min-identity"},
#endif
#ifdef BUILD_RUNNIE
    {"truth-errors", 305, "errors.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"truth-errors-min-identity", 306, "permille", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-consensus", 301, "cons.fa", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-consensus-changes", 302, "changes.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-consensus-min-depth", 303, "N", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-consensus-min-identity", 304, "permille", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-pileup", 292, "pileup.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-pileup-min-identity", 293, "permille", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-mods", 294, "mods.bed", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-mods-hi", 295, "byte", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-mods-lo", 296, "byte", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-mods-min-identity", 297, "permille", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-mods-motif", 298, "CG|C", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-mods-combine-strands", 299, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-mods-hist", 300, "hist.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map", 285, "ref.fa", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-out", 286, "hits.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-window", 287, "W", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-max-error", 288, "permille", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-records", 289, "recs.fa", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"truth-from-map", 290, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"map-sam", 291, "aln.sam", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap-from-map", 307, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"barcodes", 25, "kit.fa", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"adapters", 269, "kit.fa", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"adapter-max-dist", 270, "edits", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"trim-adapters", 271, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"adapter-window", 272, "bases", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"split-reads", 273, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"split-min-length", 274, "bases", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail", 275, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-base", 276, "letter", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-end", 277, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-window", 278, "blocks", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-min-calls", 279, "blocks", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-max-sd", 280, "sd", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-gap", 281, "windows", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-min-windows", 282, "windows", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-search", 283, "samples", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"poly-tail-min-bases", 284, "bases", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap", 31, "refs.fa", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"truth", 258, "refs.fa", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap-events", 261, "events.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap-mods", 262, "mods.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap-variants", 265, "vars.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap-variants-out", 266, "calls.tsv", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap-variants-context", 267, "N", OPTION_HIDDEN, "(flappie's option: refused here)"},
    {"remap-variants-all-paths", 268, 0, OPTION_HIDDEN, "(flappie's option: refused here)"},
#endif
    {0}
};

#ifdef BUILD_RUNNIE
/* runnie.c:71: the run-length model; its --format/--model/--trace/--reverse options are commented out in the
 * reference (runnie.c:42-60) and are ignored here with a warning */
#define DEFAULT_MODEL RUNNIE_MODEL_R941_NATIVE
#else
#define DEFAULT_MODEL FLAPPIE_MODEL_R941_NATIVE
#endif

static struct {
    int compression_level, compression_chunk_size;
    float delta;
    char *trace;
    enum flappie_outformat_type outformat;
    int limit;
    enum model_type model;
    FILE *output;
    char *prefix;
    bool reverse;
    float temperature;
    int trim_start, trim_end, varseg_chunk;
    float varseg_thresh;
    bool viterbi_only;
    char **files;
    bool uuid;
    int batch;
    int readers;
    int shard, nshard;
    bool shard_by_size;
    bool fasta, rlc, run_scale_set;     /* runnie: --fasta, --rlc, --run-scale given */
    double run_scale[4];
    bool modbase_tags;                  /* flappie: --modbase-tags given */
    bool emit_moves;                    /* flappie: --emit-moves given */
    char *barcodes;                     /* flappie: --barcodes kit file; window, max_dist, min_sep (-1: the defaults), both ends, trim */
    int bc_window, bc_max_dist, bc_min_sep;
    bool bc_both, bc_trim, bc_opts;     /* bc_opts: one of the other barcode options was given */
    char *remap, *remap_out;            /* flappie: --remap refs file, --remap-out table; the band's half-width */
    char *remap_events;                 /* ... and --remap-events table */
    int remap_band;
    bool remap_band_set;
    char *truth, *truth_out;            /* flappie: --truth refs file, --truth-out table; the band's half-width */
    int truth_band;
    bool truth_band_set;
} args = { 1, 200, 0.0f, NULL, FLAPPIE_OUTFORMAT_FASTQ, 0, DEFAULT_MODEL, NULL, "", false, 1.0f, 200, 10, 100, 0.0f, false, NULL, true, 0, 4, 0, 0, false, false, false, false,
           { 1.02, 1.04, 1.04, 1.02 }, false, false, NULL, 150, -1, -1, false, false, false, NULL, NULL, NULL, 2048, false, NULL, NULL, FLAPPIE_TRUTH_BAND_DEFAULT, false };      /* batch 0: by model (below); nshard 0: --shard not given */

/* flappie: --remap-mods table, --remap-mods-context, --remap-mods-all-paths */
static char *mods_path = NULL;
#ifndef BUILD_RUNNIE
static int mods_context = 15;
static bool mods_context_set = false, mods_all_paths = false;
#endif

/* flappie: --map reference file, --map-out table, --map-records file, --map-window and --map-max-error (-1: the defaults) (runnie: seen, to be refused);
 * map_opts: one of the options that go with --map was given */
static char *map_path = NULL, *map_out_path = NULL, *map_recs_path = NULL;
static bool map_opts = false;
/* flappie: --truth-from-map and the file of --map-sam (runnie: seen, to be refused) */
static bool tfm_on = false;
/* flappie: --remap-from-map (runnie: seen, to be refused) */
static bool rfm_on = false;
static char *tfm_sam_path = NULL;
/* flappie: the file of --map-pileup and --map-pileup-min-identity (-1: not given) (runnie: seen, to be refused) */
static char *pu_path = NULL;
static int pu_min_identity = -1;
/* flappie: the file of --map-mods, its thresholds and min identity (-1: not given), its motif (NULL: not given), --map-mods-combine-strands and the file of
 * --map-mods-hist (runnie: seen, to be refused) */
static char *mm_path = NULL, *mm_hist_path = NULL, *mm_motif = NULL;
static int mm_hi = -1, mm_lo = -1, mm_min_identity = -1;
static bool mm_combine = false;
/* flappie: the files of --map-consensus and --map-consensus-changes, --map-consensus-min-depth and -min-identity (-1: not given) (runnie: seen, to be refused) */
static char *cs_path = NULL, *cs_changes_path = NULL;
static int cs_min_depth = -1, cs_min_identity = -1;
/* flappie: the file of --truth-errors and --truth-errors-min-identity (-1: not given) (runnie: seen, to be refused) */
static char *ep_path = NULL;
static int ep_min_identity = -1;
static int map_window = -1;
#ifndef BUILD_RUNNIE
static int map_max_error = -1;
#endif

/* flappie: --adapters kit file, --adapter-max-dist (-1: the default), --trim-adapters, --adapter-window, --split-reads, --split-min-length (runnie: seen, to be
 * refused); ad_opts: one of the options that go with --adapters was given */
static char *ad_path = NULL;
static bool ad_opts = false;
static int ad_window = 150;
static long ad_min_length = 200;
static bool ad_trim = false, ad_split = false;
#ifndef BUILD_RUNNIE
static int ad_max_dist = -1;
static bool ad_window_set = false, ad_min_length_set = false;
#endif

/* flappie: --poly-tail and its options (runnie: seen, to be refused); pt_opts: one of the options that go with --poly-tail was given; pt_err: the first
 * refusal of a value, reported once every option is read (the options' order on the command line does not matter) */
static bool pt_on = false, pt_opts = false;
static flappie_polytail_summary pt_sum;
#ifndef BUILD_RUNNIE
static ffhip_polytail_params pt_params;
static flappie_polytail_opts pt_o = { 0, 0, 8, -1, 2, 5, 20000, 20, 0.3f };
static char pt_err[256];
#endif

/* flappie: --remap-variants file and table, --remap-variants-context, --remap-variants-all-paths (runnie: seen, to be refused) */
static char *vars_path = NULL, *vars_out_path = NULL;
static bool vars_opts = false;
#ifndef BUILD_RUNNIE
static int vars_context = 10;
static bool vars_all_paths = false;
#endif

static void print_models(FILE *fh) {
    for (int mdl = 0; mdl < (int)flappie_nmodel; mdl++)
        fprintf(fh, "%10s : %s  %s\n", flappie_model_string(mdl), flappie_model_description(mdl), (DEFAULT_MODEL == mdl) ? "(default)" : "");
}

static error_t parse_arg(int key, char *arg, struct argp_state *state) {
    char *next_tok = NULL;
    switch (key) {
    case 'd': args.delta = atof(arg); break;
    case 'f':
        args.outformat = get_outformat(arg);
        if (FLAPPIE_OUTFORMAT_INVALID == args.outformat) errx(EXIT_FAILURE, "Unrecognised output format \"%s\".", arg);
        break;
    case 'l': args.limit = atoi(arg); break;
    case 'm':
#ifdef BUILD_RUNNIE
        /* runnie has one model (runnie.c:71); its --model option is commented out in the reference (runnie.c:42-60): a
         * flip-flop model name here must not reach the run-length record formatter */
        warnx("--model is ignored by runnie (always %s)", flappie_model_string(DEFAULT_MODEL));
        break;
#endif
        if (0 == strcasecmp(arg, "help")) { print_models(stdout); exit(EXIT_SUCCESS); }
        args.model = get_flappie_model_type(arg);
        if (FLAPPIE_MODEL_INVALID == args.model || args.model > FLAPPIE_MODEL_INVALID) {
            fprintf(stdout, "Invalid Flappie model \"%s\".\n", arg);
            print_models(stdout);
            exit(EXIT_FAILURE);
        }
        break;
    case 'o':
        args.output = fopen(arg, "w");
        if (NULL == args.output) errx(EXIT_FAILURE, "Failed to open \"%s\" for output.", arg);
        break;
    case 'p': args.prefix = arg; break;
    case 'r': args.reverse = true; break;
    case 't':
        args.trim_start = atoi(strtok(arg, ":"));
        next_tok = strtok(NULL, ":");
        args.trim_end = (NULL != next_tok) ? atoi(next_tok) : args.trim_start;
        if (args.trim_start < 0 || args.trim_end < 0) errx(EXIT_FAILURE, "--trim values must be non-negative");
        break;
    case 'T': args.trace = arg; break;
    case 'v': args.viterbi_only = true; break;
    case 3:
        args.varseg_chunk = atoi(strtok(arg, ":"));
        next_tok = strtok(NULL, ":");
        if (NULL == next_tok) errx(EXIT_FAILURE, "--segmentation should be of form chunk:percentile");
        args.varseg_thresh = atof(next_tok) / 100.0;
        if (args.varseg_chunk < 2 || !(args.varseg_thresh >= 0.0f && args.varseg_thresh < 1.0f)) errx(EXIT_FAILURE, "--segmentation out of range");
        break;
    case 6: args.reverse = false; break;
    case 7:
        args.temperature = atof(arg);
        if (!(isfinite(args.temperature) && args.temperature > 0.0f)) errx(EXIT_FAILURE, "--temperature must be positive");
        break;
    case 8:
    case 9: args.viterbi_only = false; break;
    case 10:
    case 11:
        /* The reference prints Oxford Nanopore's licence text (flappie_licence.h).  This program is an
         * independent implementation of the same interface; it points at the respective licence files. */
        puts("This MI355X/HIP basecaller is an independent implementation of the flappie command line interface.\n"
             "The flappie reference implementation and its models are (c) Oxford Nanopore Technologies, Ltd. and are\n"
             "distributed under the Oxford Nanopore Technologies, Ltd. Public License v1.0 (see LICENCE.txt of\n"
             "https://github.com/nanoporetech/flappie); models loaded by this program remain under that licence.");
        exit(EXIT_SUCCESS);
    case 12:
        args.compression_level = atoi(arg);
        if (args.compression_level < 0 || args.compression_level > 9) errx(EXIT_FAILURE, "--hdf5-compression must be 0..9");
        break;
    case 13:
        args.compression_chunk_size = atoi(arg);
        if (args.compression_chunk_size <= 0) errx(EXIT_FAILURE, "--hdf5-chunk must be positive");
        break;
    case 14: args.uuid = true; break;
    case 15: args.uuid = false; break;
    case 16:
        args.batch = atoi(arg);
        if (args.batch <= 0) errx(EXIT_FAILURE, "--batch must be positive");
        break;
    case 17:
        args.readers = atoi(arg);
        if (args.readers < 0 || args.readers > 64) errx(EXIT_FAILURE, "--readers must be between 0 and 64");
        break;
    case 18:
        if (2 != sscanf(arg, "%d/%d", &args.shard, &args.nshard) || args.nshard < 1 || args.shard < 0 || args.shard >= args.nshard)
            errx(EXIT_FAILURE, "--shard takes g/n with 0 <= g < n");
        break;
    case 19: args.shard_by_size = true; break;
#ifdef BUILD_RUNNIE
    case 20: args.fasta = true; break;
    case 21: args.rlc = true; break;
    case 22: {
        char *p = arg;
        for (int k = 0; k < 4; k++) {
            char *end;
            args.run_scale[k] = strtod(p, &end);
            if (end == p || !(args.run_scale[k] > 0.0) || !isfinite(args.run_scale[k]) || *end != (k < 3 ? ',' : 0))
                errx(EXIT_FAILURE, "--run-scale takes four positive factors A,C,G,T");
            p = end + 1;
        }
        args.run_scale_set = true;
        break;
    }
#else
    case 23: args.modbase_tags = true; break;
    case 24: args.emit_moves = true; break;
#endif
    case 25: args.barcodes = arg; break;
    case 31: args.remap = arg; break;
    case 258: args.truth = arg; break;
    case 261: args.remap_events = arg; break;
    case 262: mods_path = arg; break;
    case 265: vars_path = arg; break;
    case 269: ad_path = arg; break;
    case 275: pt_on = true; break;
#ifdef BUILD_RUNNIE
    case 276: case 277: case 278: case 279: case 280: case 281: case 282: case 283: case 284: pt_opts = true; break;
#else
    case 277: pt_o.from_end = 1; pt_opts = true; break;
    case 276: case 278: case 279: case 280: case 281: case 282: case 283: case 284: {
        static const char *const names[] = { "base", NULL, "window", "min-calls", "max-sd", "gap", "min-windows", "search", "min-bases" };
        char why[256];
        pt_opts = true;
        if (0 != flappie_polytail_set(&pt_o, names[key - 276], arg, why, sizeof why) && 0 == pt_err[0]) snprintf(pt_err, sizeof pt_err, "%s", why);
        break;
    }
#endif
    case 285: map_path = arg; break;
    case 286: map_out_path = arg; map_opts = true; break;
    case 289: map_recs_path = arg; map_opts = true; break;
    case 290: tfm_on = true; break;
    case 307: rfm_on = true; break;
    case 291: tfm_sam_path = arg; break;
    case 292: pu_path = arg; break;
    case 293: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || v < 0 || v > 1000) errx(EXIT_FAILURE, "--map-pileup-min-identity must be a whole number from 0 to 1000");
        pu_min_identity = (int)v;
        break;
    }
    case 294: mm_path = arg; break;
    case 295: case 296: case 297: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10), top = key == 297 ? 1000 : 255;
        if (end == arg || *end != '\0' || v < 0 || v > top)
            errx(EXIT_FAILURE, "--map-mods-%s must be a whole number from 0 to %ld", key == 295 ? "hi" : key == 296 ? "lo" : "min-identity", top);
        *(key == 295 ? &mm_hi : key == 296 ? &mm_lo : &mm_min_identity) = (int)v;
        break;
    }
    case 298:
        if (0 != strcmp(arg, "CG") && 0 != strcmp(arg, "C")) errx(EXIT_FAILURE, "--map-mods-motif is CG or C, not \"%s\"", arg);
        mm_motif = arg;
        break;
    case 299: mm_combine = true; break;
    case 300: mm_hist_path = arg; break;
    case 301: cs_path = arg; break;
    case 302: cs_changes_path = arg; break;
    case 303: case 304: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10), low = key == 303 ? 1 : 0, top = key == 303 ? 65535 : 1000;
        if (end == arg || *end != '\0' || v < low || v > top)
            errx(EXIT_FAILURE, "--map-consensus-%s must be a whole number from %ld to %ld", key == 303 ? "min-depth" : "min-identity", low, top);
        *(key == 303 ? &cs_min_depth : &cs_min_identity) = (int)v;
        break;
    }
    case 305: ep_path = arg; break;
    case 306: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || v < 0 || v > 1000) errx(EXIT_FAILURE, "--truth-errors-min-identity must be a whole number from 0 to 1000");
        ep_min_identity = (int)v;
        break;
    }
#ifdef BUILD_RUNNIE
    case 287: case 288: map_opts = true; break;
    case 270: case 271: case 272: case 273: case 274: ad_opts = true; break;
#else
    case 287: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || v < 64 || v > FFHIP_MAP_MAX_ANCHOR) errx(EXIT_FAILURE, "--map-window must be a whole number from 64 to %d", FFHIP_MAP_MAX_ANCHOR);
        map_window = (int)v; map_opts = true;
        break;
    }
    case 288: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || v < 0 || v > 500) errx(EXIT_FAILURE, "--map-max-error must be a whole number from 0 to 500");
        map_max_error = (int)v; map_opts = true;
        break;
    }
    case 270: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || v < 0 || v > 63) errx(EXIT_FAILURE, "--adapter-max-dist must be a whole number from 0 to 63");
        ad_max_dist = (int)v; ad_opts = true;
        break;
    }
    case 271: ad_trim = true; ad_opts = true; break;
    case 272: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || v < 0 || v > 1000000) errx(EXIT_FAILURE, "--adapter-window must be a whole number from 0 to 1000000");
        ad_window = (int)v; ad_window_set = true; ad_opts = true;
        break;
    }
    case 273: ad_split = true; ad_opts = true; break;
    case 274: {
        char *end = NULL;
        const long v = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || v < 0 || v > 1000000000) errx(EXIT_FAILURE, "--split-min-length must be a whole number from 0 to 1000000000");
        ad_min_length = v; ad_min_length_set = true; ad_opts = true;
        break;
    }
#endif
    case 266: vars_out_path = arg; break;
#ifdef BUILD_RUNNIE
    case 267: case 268: vars_opts = true; break;
#else
    case 267: {
        char *end = NULL;
        const long c = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || c < 1 || c > 23) errx(EXIT_FAILURE, "--remap-variants-context must be a whole number from 1 to 23");
        vars_context = (int)c; vars_opts = true;
        break;
    }
    case 268: vars_all_paths = true; vars_opts = true; break;
    case 263: {
        char *end = NULL;
        const long c = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || c < 0 || c > 31) errx(EXIT_FAILURE, "--remap-mods-context must be a whole number from 0 to 31");
        mods_context = (int)c; mods_context_set = true;
        break;
    }
    case 264: mods_all_paths = true; break;
    case 256: args.remap_out = arg; break;      /* (keys above UCHAR_MAX: argp makes a short option of a printable one) */
    case 257: {
        char *end = NULL;
        const long w = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || w < 0 || w > FLAPPIE_REMAP_BAND_MAX) errx(EXIT_FAILURE, "--remap-band must be a whole number from 0 to %d", FLAPPIE_REMAP_BAND_MAX);
        args.remap_band = (int)w; args.remap_band_set = true;
        break;
    }
    case 259: args.truth_out = arg; break;
    case 260: {
        char *end = NULL;
        const long w = strtol(arg, &end, 10);
        if (end == arg || *end != '\0' || w < 0 || w > FLAPPIE_TRUTH_BAND_MAX) errx(EXIT_FAILURE, "--truth-band must be a whole number from 0 to %d", FLAPPIE_TRUTH_BAND_MAX);
        args.truth_band = (int)w; args.truth_band_set = true;
        break;
    }
#endif
#ifndef BUILD_RUNNIE
    case 26:
        args.bc_window = atoi(arg); args.bc_opts = true;
        if (args.bc_window < 1 || args.bc_window > 256) errx(EXIT_FAILURE, "--barcode-window must be between 1 and 256");
        break;
    case 27:
        args.bc_max_dist = atoi(arg); args.bc_opts = true;
        if (args.bc_max_dist < 0 || args.bc_max_dist > 255) errx(EXIT_FAILURE, "--barcode-max-dist must be between 0 and 255");
        break;
    case 28:
        args.bc_min_sep = atoi(arg); args.bc_opts = true;
        if (args.bc_min_sep < 0 || args.bc_min_sep > 255) errx(EXIT_FAILURE, "--barcode-min-sep must be between 0 and 255");
        break;
    case 29: args.bc_both = true; args.bc_opts = true; break;
    case 30: args.bc_trim = true; args.bc_opts = true; break;
#endif
    case ARGP_KEY_NO_ARGS: argp_usage(state); break;
    case ARGP_KEY_ARG:
        args.files = &state->argv[state->next - 1];
        state->next = state->argc;
        break;
    default: return ARGP_ERR_UNKNOWN;
    }
    return 0;
}

static struct argp argp = { options, parse_arg, args_doc, doc };

/* this libhdf5 is not built thread-safe: every HDF5 call of either thread is made under this lock */
static pthread_mutex_t hdf5_lock = PTHREAD_MUTEX_INITIALIZER;

/* FLAPPIE_CLI_TIMING=1: wall-clock split of the driver's phases on stderr at exit */
static double t_phase[8];
static const char *phase_name[8] = { "fast5 read", "signal preparation", "batch create/destroy", "upload+network+decode", "fetch results", "write output",
                                     "  of which set_prepared", "  of which batch_run" };
/* Development switches of the binary: FLAPPIE_DEBUG=token[,token=value ...] -- no_reader_thread, no_writer_thread,
 * list_only, kill_reader=k:f, no_numa_bind, sysfs_root=DIR.  NULL when the token is absent, its value ("" for a bare token) otherwise. */
static const char *cli_dbg(const char *token) {
    static char buf[256];
    const char *e = getenv("FLAPPIE_DEBUG");
    const size_t n = strlen(token);
    while (e && *e) {
        const char *end = e + strcspn(e, ", ;");
        if ((size_t)(end - e) >= n && 0 == strncmp(e, token, n) && (e + n == end || '=' == e[n])) {
            const size_t vl = (e + n == end) ? 0 : (size_t)(end - e - n - 1);
            if (vl >= sizeof buf) return NULL;
            memcpy(buf, e + n + 1, vl);
            buf[vl] = 0;
            return buf;
        }
        e = *end ? end + 1 : end;
    }
    return NULL;
}

/* This process, the reader children it is about to fork and the pinned staging they fill, on the CPUs of the GPU's NUMA node (eight
 * ranks of a node otherwise read their files wherever the scheduler puts them).  The node comes from sysfs -- the HIP runtime must not be up before the
 * fork --: the device-th render node of vendor 0x1002 in minor order, the device number first taken through the *_VISIBLE_DEVICES variables (physical_gpu_index).  Left alone when the
 * node is unknown or none of its CPUs is in this process's set; FLAPPIE_DEBUG=no_numa_bind switches it off, sysfs_root=DIR is for the tests. */
/* HIP device number of this process -> position among the node's GPUs in the kernel's order, through HIP_VISIBLE_DEVICES (or its synonym
 * CUDA_VISIBLE_DEVICES) and ROCR_VISIBLE_DEVICES below it; -1 when an entry is not a plain number (a UUID) or the index is beyond the list -- the process
 * is then left unbound: several ranks pinned to ONE socket by a wrong guess are worse off than unbound ones (shard.py physical_gpu_index) */
static int physical_gpu_index(int device) {
    const char *hip = getenv("HIP_VISIBLE_DEVICES");
    const char *names[2] = { (hip && hip[0]) ? "HIP_VISIBLE_DEVICES" : "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES" };
    for (int v = 0; v < 2; v++) {
        const char *text = getenv(names[v]);
        if (NULL == text || 0 == text[strspn(text, " ")]) continue;
        const char *p = text;
        for (int k = 0; k < device; k++) {
            p = strchr(p, ',');
            if (NULL == p) return -1;
            p++;
        }
        p += strspn(p, " ");
        char *end;
        const long val = strtol(p, &end, 10);
        if (end == p || (end[strspn(end, " ")] != ',' && end[strspn(end, " ")] != 0) || val < 0) return -1;
        device = (int)val;
    }
    return device;
}

static int bind_to_gpu_numa(int device) {
    device = physical_gpu_index(device);
    if (device < 0) return -1;
    const char *root = cli_dbg("sysfs_root");
    char sys[256], path[512], buf[4096];
    snprintf(sys, sizeof sys, "%s", (root && root[0]) ? root : "/sys");
    int minors[64], nodes[64], n = 0;
    snprintf(path, sizeof path, "%s/class/drm", sys);
    DIR *d = opendir(path);
    if (NULL == d) return -1;
    for (struct dirent *e; n < 64 && NULL != (e = readdir(d));) {
        int minor;
        if (1 != sscanf(e->d_name, "renderD%d", &minor)) continue;
        snprintf(path, sizeof path, "%s/class/drm/%s/device/vendor", sys, e->d_name);
        FILE *fh = fopen(path, "r");
        if (NULL == fh) continue;
        const int amd = (NULL != fgets(buf, sizeof buf, fh) && 0 == strncasecmp(buf, "0x1002", 6));
        fclose(fh);
        if (!amd) continue;
        snprintf(path, sizeof path, "%s/class/drm/%s/device/numa_node", sys, e->d_name);
        int node = -1;
        if (NULL != (fh = fopen(path, "r"))) { if (1 != fscanf(fh, "%d", &node)) node = -1; fclose(fh); }
        int k = n++;
        while (k > 0 && minors[k - 1] > minor) { minors[k] = minors[k - 1]; nodes[k] = nodes[k - 1]; k--; }
        minors[k] = minor; nodes[k] = node;
    }
    closedir(d);
    if (device < 0 || device >= n || nodes[device] < 0) return -1;
    snprintf(path, sizeof path, "%s/devices/system/node/node%d/cpulist", sys, nodes[device]);
    FILE *fh = fopen(path, "r");
    if (NULL == fh) return -1;
    const int got = NULL != fgets(buf, sizeof buf, fh);
    fclose(fh);
    if (!got) return -1;
    cpu_set_t mine, want;
    if (0 != sched_getaffinity(0, sizeof mine, &mine)) return -1;
    CPU_ZERO(&want);
    int nbound = 0;
    for (char *p = buf; *p && *p != '\n';) {
        char *end;
        const long lo = strtol(p, &end, 10);
        long hi = lo;
        if (end == p) break;
        if ('-' == *end) { p = end + 1; hi = strtol(p, &end, 10); }
        for (long c = lo; c <= hi && c < CPU_SETSIZE; c++) if (CPU_ISSET((int)c, &mine)) { CPU_SET((int)c, &want); nbound++; }
        p = (',' == *end) ? end + 1 : end;
    }
    if (0 == nbound || 0 != sched_setaffinity(0, sizeof want, &want)) return -1;
    if (getenv("FLAPPIE_CLI_TIMING")) fprintf(stderr, "bound to %d CPUs of NUMA node %d (GPU %d)\n", nbound, nodes[device], device);
    return nodes[device];
}

static double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }
static double t_program_start;          /* main's first statement (FLAPPIE_DEBUG=pack_log's time stamps) */
/* what the run basecalled: reads, samples of their trimmed ranges (the metric of SURVEY.md section 8d), samples read from the files */
static unsigned long long n_called_reads, n_called_samples, n_raw_samples;
static unsigned long long n_lost_reads;  /* reads of batches that failed and could not be called another way: the exit status says so */
/* what the batches cost: a batch (a launch per layer) takes as long as its longest read needs whatever the others' lengths, a read tile of 16 as long as
 * ITS longest read holds its workgroups -- samples submitted against samples x slots paid for, at both grains (FLAPPIE_CLI_TIMING prints them) */
static unsigned long long n_batches, n_packed_batches, n_batch_samples, n_batch_slot_samples, n_tile_slot_samples;
static int reader_failures;              /* reader children that ended abnormally: the exit status says so */

typedef struct {
    char *filename;                     /* owned */
    struct _raw_basecall_info res;      /* rt filled by read_raw, start/end by the preparation; basecall == NULL until called */
    int prepared;                       /* index into the chunk's ffhip_prep, or -1 */
    char *rle_text;                     /* runnie: the read's records, formatted (runnie.c:282-313); --fasta: its sequence, wrapped */
    uint8_t *ml;                        /* --modbase-tags: the 5mC byte of every called base, aligned with res.basecall (owned) */
    uint8_t *mv;                        /* --emit-moves: the move byte of every block, in signal order (owned); res.pos holds the block of every base */
    int mv_stride;                      /* ... the samples a block */
    float sm, sd;                       /* ... the median and MAD the read was normalised with */
    ffhip_barcode_call bc;              /* --barcodes: the read's record */
    int have_bc;
    ffhip_adapter_header ad_head;       /* --adapters: the read's record */
    ffhip_adapter_hit ad_hits[FFHIP_ADAPTER_MAX_HITS];
    int have_ad;
    ffhip_map_call mp;                  /* --map: the read's record */
    int have_mp;
    ffhip_polytail pt;                  /* --poly-tail: the read's record */
    int have_pt;
    int rm_ref;                         /* --remap: the read's record of the sequences (-1: none), and what the batch returned for it */
    int have_rm, rm_status;
    size_t rm_L, rm_nblock;
    float rm_score;
    uint8_t *rm;                        /* ... its moves (owned; NULL unless mapped) */
    ffhip_event *ev;                    /* --remap-events: its rm_L events (owned; NULL unless mapped) */
    ffhip_site_mod *smods;               /* --remap-mods: its nsm site records (owned; NULL unless mapped) */
    size_t nsmods;
    ffhip_variant_call *vcalls;          /* --remap-variants: its nvcalls records (owned; NULL unless mapped and with variants) */
    size_t nvcalls;
    int tr_ref, have_tr;                /* --truth: the read's record of the truths (-1: none), and what the batch returned for it */
    flappie_truth_rec tr;
    uint8_t *tr_ops;                    /* ... its ops (owned; NULL unless aligned) */
    size_t tr_nops;
    int rle_nocall;                     /* runnie --fasta: no runs, or a failed run-length estimate (decode_runnie.py: "No basecall returned") */
    /* a read of a MULTI-READ file: its samples as the file holds them (owned; res.rt.raw stays NULL, res.rt.n counts them) and its calibration -- the
     * preparation scales them on the device (ffhip_prep_begin_dac) */
    int from_multi;
    int16_t *dac;
    float dac_offset, dac_unit;
} item;
static int item_has_signal(const item *it) { return NULL != it->res.rt.raw || NULL != it->dac; }

/* Batch objects own gigabytes of workspace; creating one per group costs more than running it.  Full-size groups
 * (--batch reads) share one cached object whose capacity grows when a longer read turns up. */
#define NINFLIGHT 3                    /* batches submitted and not collected, at most (FLAPPIE_INFLIGHT=3; default 2) */
static struct { ffhip_batch *b; int nread; size_t cap; } batch_cache[NINFLIGHT];

/* *nslot = reads the returned batch was created for: args.batch for the cached objects (groups of at least a quarter of
 * that are padded with empty slots), the group's own size for small groups */
static ffhip_batch *acquire_batch(struct ffhip_engine *eng, const struct ffhip_model *mdl, int n, size_t len, int slot, int *cached, int *nslot) {
    *cached = 0;
    *nslot = n;
    if (4 * n < args.batch) return ffhip_batch_create(eng, mdl, n, len);
    if (NULL == batch_cache[slot].b || batch_cache[slot].cap < len) {
        if (batch_cache[slot].b) ffhip_batch_destroy(batch_cache[slot].b);
        batch_cache[slot].cap = len + len / 8;
        batch_cache[slot].nread = args.batch;
        batch_cache[slot].b = ffhip_batch_create(eng, mdl, args.batch, batch_cache[slot].cap);
        if (NULL == batch_cache[slot].b) { batch_cache[slot].cap = 0; return NULL; }
    }
    *cached = 1;
    *nslot = args.batch;
    return batch_cache[slot].b;
}

/* Packed batches (ffhip.h "packed batches"): reads of mixed lengths, several to a row.  One cached object per pipeline slot, `--batch` rows of the chunk's row
 * capacity, created anew when a chunk needs longer rows. */
static struct { ffhip_batch *b; size_t cap; int max_reads, rows, full, single; } pack_cache[NINFLIGHT];
static ffhip_batch *acquire_packed(struct ffhip_engine *eng, const struct ffhip_model *mdl, int rows, int rows_full, size_t cap, int max_reads, int slot, int single) {
    /* (an object with MORE rows or longer rows than this batch needs serves it as it is: rows without a read cost nothing, and re-creating a 90 GB object is seconds) */
    if (NULL == pack_cache[slot].b || pack_cache[slot].cap < cap || pack_cache[slot].max_reads < max_reads || pack_cache[slot].rows < rows) {
        if (pack_cache[slot].b) ffhip_batch_destroy(pack_cache[slot].b);
        /* two shapes of object only, so that a slot's object is re-created when the reads get LONGER and for nothing else: a quarter of the rows for a run's first,
         * small chunk (created in a fraction of a second, replaced by the second chunk), all the rows the memory takes otherwise; capacities in pack_row_cap's steps */
        const int make_rows = (4 * rows <= rows_full) ? (rows_full / 4 + 15) / 16 * 16 : rows_full;
        pack_cache[slot].cap = cap;
        pack_cache[slot].max_reads = max_reads;
        pack_cache[slot].rows = make_rows;
        pack_cache[slot].full = (make_rows == rows_full);
        pack_cache[slot].single = single;
        const double tc0 = now_s();
        pack_cache[slot].b = cli_dbg("pack_fail") ? NULL : ffhip_batch_create_packed(eng, mdl, make_rows, cap, max_reads);      /* (pack_fail: tests -- as if the device had no memory for it) */
        if (getenv("FLAPPIE_CLI_TIMING")) fprintf(stderr, "packed batch object (slot %d): %d rows of %zu samples, up to %d reads%s, %.2f s\n", slot, make_rows, cap, max_reads,
                                                  pack_cache[slot].b ? "" : " -- FAILED", now_s() - tc0);
        if (NULL == pack_cache[slot].b) { pack_cache[slot].cap = 0; return NULL; }
    }
    return pack_cache[slot].b;
}
/* row capacities in steps of a quarter octave (a batch object is re-created -- seconds of hipMalloc at these sizes -- only when a chunk needs the next step) */
static size_t pack_row_cap(size_t want) {
    size_t c = 4096;
    while (c < want) c = (c + c / 4 + 1023) & ~(size_t)1023;
    return c;
}

/* A group of prepared reads in flight: submitted (upload + network + decode enqueued on the batch's stream), collected
 * later (flappie.c:264-316 after normalisation) -- so the host side of the next group overlaps the GPU side of this one. */
struct chunk_ctx;
typedef struct { ffhip_batch *b; int cached, n, *idx; item **its; const ffhip_prep *prep; struct chunk_ctx *owner; int packed; } pending_batch;
/* flappie --barcodes: the kit as the file gave it and on the device; reads per barcode, the last entry the unclassified ones */
static flappie_barcode_kit *bc_kit = NULL;
static ffhip_barcodes *bc_dev = NULL;
static unsigned long long bc_count[FLAPPIE_BARCODE_MAX_KIT + 1];
/* flappie --adapters: likewise; kept hits per adapter, reads with a hit, and what --split-reads did (reads split, pieces written, pieces dropped, reads with more
 * than 15 hits) */
static flappie_adapter_kit *ad_kit = NULL;
static ffhip_adapters *ad_dev = NULL;
static unsigned long long ad_count[FLAPPIE_ADAPTER_MAX_KIT], ad_reads_with_hit, ad_stats[4];
/* flappie --map: the reference as the file gave it and on the device, the table, the records' file, and the summary */
static flappie_map_ref *mp_ref = NULL;
static ffhip_map_ref *mp_dev = NULL;
static FILE *mp_out = NULL, *mp_recs = NULL;
static flappie_map_summary mp_sum;
/* flappie --remap: the sequences, the table, and the summary's counts: mapped, no record, refused, mapped with maxdev = band */
static flappie_remap_refs *rm_refs = NULL;
static FILE *rm_out = NULL;
static unsigned long long rm_count[4];
/* flappie --remap-events: the table, and the summary's counts: reads and bases written */
static FILE *ev_out = NULL;
static unsigned long long ev_count[2];
/* --remap-events: a mapped read's lines of events.tsv: name, base index, base letter, first raw sample, samples, mean, sd */
static void write_events(FILE *out, const char *name, const uint8_t *codes, const char *alphabet, size_t trim_start, const ffhip_event *ev, size_t L) {
    for (size_t i = 0; i < L; i++)
        fprintf(out, "%s\t%zu\t%c\t%zu\t%d\t%.9g\t%.9g\n", name, i, alphabet[codes[i]], trim_start + (size_t)ev[i].first, (int)ev[i].count, (double)ev[i].mean, (double)ev[i].sd);
}
/* flappie --remap-mods: the table, and the summary's counts: reads and sites written */
static FILE *md_out = NULL;
static unsigned long long md_count[2];
/* flappie --remap-variants: the variants, the table, the records whose variants were written, and the summary's counts: reads and variants written */
static flappie_variants *vr_vars = NULL;
static FILE *vr_out = NULL;
static unsigned char *vr_done = NULL;
static unsigned long long vr_count[2];
/* flappie --truth: the truths, the table, and the summary */
static flappie_remap_refs *tr_refs = NULL;
static FILE *tr_out = NULL;
static flappie_truth_summary tr_sum;
/* flappie --truth-from-map: the truths are the mapped stretches (tr_refs stays NULL; tr_out and tr_sum serve); the file of --map-sam */
static FILE *tfm_sam = NULL;
#ifdef BUILD_RUNNIE
/* --fasta: the runs and their run-length estimates come from the device (FFHIP_RUN_RLE_RUNS) with the batch's scale factors */
static unsigned run_flags(void) { return (args.viterbi_only ? FFHIP_RUN_VITERBI_ONLY : 0u) | (args.trace ? 0u : FFHIP_RUN_NO_TRACE) | (args.fasta ? FFHIP_RUN_RLE_RUNS : 0u); }
static int batch_run(ffhip_batch *b, unsigned flags, item **its, int n) {
    if (args.fasta) { const int rc = ffhip_batch_set_run_scale(b, args.run_scale); if (rc) return rc; }
    return ffhip_batch_run(b, args.temperature, flags);
}
#else
/* flappie --map-pileup: the one pileup of the run, attached to every batch object and downloaded once at the end; its table */
static ffhip_pileup *pu_dev = NULL;
static FILE *pu_out = NULL;
/* flappie --map-mods: likewise the one mod pileup of the run; its table and the histogram's file */
static ffhip_modpileup *mm_dev = NULL;
static FILE *mm_out = NULL, *mm_hist = NULL;
/* flappie --map-consensus: likewise the one consensus of the run; its FASTA file and the table of changes */
static ffhip_consensus *cs_dev = NULL;
static FILE *cs_out = NULL, *cs_changes = NULL;
/* flappie --truth-errors: likewise the one error profile of the run, in either truth mode; its table */
static ffhip_errprofile *ep_dev = NULL;
static FILE *ep_out = NULL;
/* --modbase-tags: the 5mC bytes of the called bases come from the device (FFHIP_RUN_MOD_PROBS); --emit-moves: the move table does (FFHIP_RUN_MOVES);
 * --barcodes: the reads' barcode records do (FFHIP_RUN_BARCODES); --adapters: their adapter records (FFHIP_RUN_ADAPTERS); --poly-tail: their poly tail
 * records (FFHIP_RUN_POLYTAIL) */
static unsigned run_flags(void) {
    return (args.viterbi_only ? FFHIP_RUN_VITERBI_ONLY : 0u) | (args.trace ? 0u : FFHIP_RUN_NO_TRACE) | ((args.modbase_tags || mm_dev) ? FFHIP_RUN_MOD_PROBS : 0u) | (mm_dev ? FFHIP_RUN_MOD_PILEUP : 0u) |
           (args.emit_moves ? FFHIP_RUN_MOVES : 0u) | (bc_dev ? FFHIP_RUN_BARCODES : 0u) | (ad_dev ? FFHIP_RUN_ADAPTERS : 0u) | (mp_dev ? FFHIP_RUN_MAP : 0u) | (pt_on ? FFHIP_RUN_POLYTAIL : 0u) | ((rm_refs || rfm_on) ? FFHIP_RUN_REMAP : 0u) | ((tr_refs || tfm_on) ? FFHIP_RUN_TRUTH : 0u) | (pu_dev ? FFHIP_RUN_PILEUP : 0u) | (cs_dev ? FFHIP_RUN_CONSENSUS : 0u) | (ep_dev ? FFHIP_RUN_ERRPROFILE : 0u) |
           (ev_out ? FFHIP_RUN_EVENTS : 0u) | (md_out ? FFHIP_RUN_REMAP_MODS : 0u) | (vr_out ? FFHIP_RUN_REMAP_VARIANTS : 0u);
}
/* --remap: every read's record, by its read id, then by its file's base name; a bad record goes as a sequence of no bases (status 2) */
static int batch_set_remap(ffhip_batch *b, item **its, int n) {
    const int nb = ffhip_batch_nreads(b);
    const uint8_t **codes = calloc(nb > 0 ? nb : 1, sizeof(uint8_t *));
    size_t *len = calloc(nb > 0 ? nb : 1, sizeof(size_t));
    static const uint8_t none = 0;
    int rc = (codes && len) ? 0 : -1;
    for (int i = 0; 0 == rc && i < n && i < nb; i++) {
        const int k = its[i]->rm_ref = flappie_remap_refs_find(rm_refs, its[i]->res.rt.uuid, its[i]->filename);
        if (k < 0) continue;
        const int bad = rm_refs->bad[k] || 0 == rm_refs->len[k];
        codes[i] = bad ? &none : rm_refs->codes[k];
        len[i] = bad ? 0 : rm_refs->len[k];
    }
    if (0 == rc) rc = ffhip_batch_set_remap(b, nb, codes, len, args.remap_band);
    if (0 == rc && md_out) rc = ffhip_batch_set_remap_mods(b, mods_context, mods_all_paths ? 1 : 0);
    if (0 == rc && vr_out) {           /* every read's variants: those of its record, in file order (a record that cannot be used has none) */
        size_t total = 0, at = 0;
        for (int i = 0; i < n && i < nb; i++) if (its[i]->rm_ref >= 0 && len[i]) total += flappie_variants_of(vr_vars, its[i]->rm_ref, NULL);
        ffhip_variant *all = malloc((total ? total : 1) * sizeof *all);
        const ffhip_variant **lists = calloc(nb > 0 ? nb : 1, sizeof *lists);
        size_t *nvar = calloc(nb > 0 ? nb : 1, sizeof *nvar);
        if (NULL == all || NULL == lists || NULL == nvar) rc = -1;
        for (int i = 0; 0 == rc && i < n && i < nb; i++) {
            if (its[i]->rm_ref < 0 || 0 == len[i]) continue;
            lists[i] = all + at;
            at += nvar[i] = flappie_variants_of(vr_vars, its[i]->rm_ref, all + at);
        }
        if (0 == rc) rc = ffhip_batch_set_remap_variants(b, nb, lists, nvar, vars_context, vars_all_paths ? 1 : 0);
        free(all);
        free(lists);
        free(nvar);
    }
    free(codes);
    free(len);
    return rc;
}
/* --truth: likewise */
static int batch_set_truth(ffhip_batch *b, item **its, int n) {
    const int nb = ffhip_batch_nreads(b);
    const uint8_t **codes = calloc(nb > 0 ? nb : 1, sizeof(uint8_t *));
    size_t *len = calloc(nb > 0 ? nb : 1, sizeof(size_t));
    static const uint8_t none = 0;
    int rc = (codes && len) ? 0 : -1;
    for (int i = 0; 0 == rc && i < n && i < nb; i++) {
        const int k = its[i]->tr_ref = flappie_remap_refs_find(tr_refs, its[i]->res.rt.uuid, its[i]->filename);
        if (k < 0) continue;
        const int bad = tr_refs->bad[k] || 0 == tr_refs->len[k];
        codes[i] = bad ? &none : tr_refs->codes[k];
        len[i] = bad ? 0 : tr_refs->len[k];
    }
    if (0 == rc) rc = ffhip_batch_set_truth(b, nb, codes, len, args.truth_band);
    free(codes);
    free(len);
    return rc;
}
static int batch_run(ffhip_batch *b, unsigned flags, item **its, int n) {
    if (bc_dev) { const int rc = ffhip_batch_set_barcodes(b, bc_dev, args.bc_max_dist, args.bc_min_sep, args.bc_both); if (rc) return rc; }
    if (ad_dev) { const int rc = ffhip_batch_set_adapters(b, ad_dev, ad_max_dist); if (rc) return rc; }
    if (mp_dev) { const int rc = ffhip_batch_set_map(b, mp_dev, map_window, map_max_error); if (rc) return rc; }
    if (pt_on) { const int rc = ffhip_batch_set_polytail(b, &pt_params); if (rc) return rc; }
    if (rm_refs) { const int rc = batch_set_remap(b, its, n); if (rc) return rc; }
    if (tr_refs) { const int rc = batch_set_truth(b, its, n); if (rc) return rc; }
    if (tfm_on) { const int rc = ffhip_batch_set_truth_from_map(b, 1, args.truth_band); if (rc) return rc; }
    if (rfm_on) { const int rc = ffhip_batch_set_remap_from_map(b, 1, args.remap_band); if (rc) return rc; }
    if (pu_dev) { const int rc = ffhip_batch_set_pileup(b, pu_dev); if (rc) return rc; }
    if (mm_dev) { const int rc = ffhip_batch_set_modpileup(b, mm_dev); if (rc) return rc; }
    if (cs_dev) { const int rc = ffhip_batch_set_consensus(b, cs_dev); if (rc) return rc; }
    if (ep_dev) { const int rc = ffhip_batch_set_errprofile(b, ep_dev); if (rc) return rc; }
    return ffhip_batch_run(b, args.temperature, flags);
}
#endif

/* n reads in the rows of one packed batch: slot_of / off_of from ffhip_pack_plan, `cap` the row capacity it was made for */
static pending_batch submit_packed(struct ffhip_engine *eng, const struct ffhip_model *mdl, const ffhip_prep *prep, item **its, int n, const int *slot_of, const int *off_of,
                                   int rows, int rows_full, size_t cap, size_t cap_obj, int max_reads, int slot, int single) {
    pending_batch pb = { NULL, 1, n, malloc((n > 0 ? n : 1) * sizeof(int)), malloc((n > 0 ? n : 1) * sizeof(item *)), prep, NULL, 1 };
    memcpy(pb.its, its, n * sizeof(item *));
    size_t longest = 0;
    unsigned long long samples = 0;
    size_t *row_end = calloc(rows, sizeof(size_t));
    for (int i = 0; i < n; i++) {
        pb.idx[i] = its[i]->prepared;
        const size_t li = its[i]->res.rt.end - its[i]->res.rt.start;
        samples += li;
        if (row_end) { const size_t e = (size_t)off_of[i] + ffhip_model_nblock(mdl, li); if (e > row_end[slot_of[i]]) row_end[slot_of[i]] = e; }
    }
    /* what the batch costs: its longest ROW (in blocks -> samples of the trimmed signal), whatever the others hold */
    const size_t nb_cap = ffhip_model_nblock(mdl, cap);
    const size_t spb = nb_cap ? (cap + nb_cap / 2) / nb_cap : 1;      /* samples a block (the model's stride) */
    for (int r = 0; row_end && r < rows; r++) {
        if (row_end[r] > longest) longest = row_end[r];
    }
    n_batches++; n_packed_batches++;
    n_batch_samples += samples;
    n_batch_slot_samples += (unsigned long long)longest * spb * (unsigned long long)(16 * ((rows + 15) / 16));
    if (cli_dbg("pack_log"))             /* development: what every packed batch holds and pays for */
        fprintf(stderr, "packed batch %llu (submitted at %.3f s): %d reads, %llu samples in %d rows planned for %zu samples (object: %d rows of %zu), longest row %zu samples, longest read %zu: fill %.3f\n", n_packed_batches, now_s() - t_program_start, n, samples,
                rows, cap, rows_full, cap_obj, longest * spb, (size_t)(its[0]->res.rt.end - its[0]->res.rt.start), (double)samples / ((double)(longest * spb) * (double)(16 * ((rows + 15) / 16))));
    for (int r0 = 0; row_end && r0 < rows; r0 += 16) {
        size_t lt = 0;
        for (int r = r0; r < rows && r < r0 + 16; r++) if (row_end[r] > lt) lt = row_end[r];
        n_tile_slot_samples += 16ull * lt * spb;
    }
    free(row_end);
    double t0 = now_s();
    pb.b = acquire_packed(eng, mdl, rows, rows_full, cap_obj, max_reads, slot, single);      /* (the object's rows come in steps; the plan was made for rows of `cap` samples) */
    t_phase[2] += now_s() - t0; t0 = now_s();
    const unsigned flags = run_flags();
    if (getenv("FLAPPIE_CLI_TIMING")) fprintf(stderr, "packed batch: %d reads, %.1f Msamples in %d rows planned for %zu samples (longest row %zu)\n", n, (double)samples / 1e6, rows, cap, longest * spb);
    int rc_sub = (NULL == pb.b) ? -1 : ffhip_batch_set_prepared_packed(pb.b, prep, n, pb.idx, slot_of, off_of);
    t_phase[6] += now_s() - t0;
    const double t1 = now_s();
    if (0 == rc_sub) rc_sub = batch_run(pb.b, flags, pb.its, n);
    t_phase[7] += now_s() - t1;
    if (0 != rc_sub) { warnx("%s", ffhip_last_error()); pb.b = NULL; }
    t_phase[3] += now_s() - t0;
    return pb;
}

static pending_batch submit_batch(struct ffhip_engine *eng, const struct ffhip_model *mdl, const ffhip_prep *prep, item **its, int n, int slot) {
    const int nmax = (n > args.batch) ? n : args.batch;
    pending_batch pb = { NULL, 0, n, malloc(nmax * sizeof(int)), malloc(n * sizeof(item *)), prep, NULL, 0 };
    memcpy(pb.its, its, n * sizeof(item *));
    for (int i = 0; i < nmax; i++) pb.idx[i] = (i < n) ? its[i]->prepared : -1;             /* -1: empty slot */
    size_t len = 0;                                          /* capacity = the longest read of the (sorted) group */
    for (int i = 0; i < n; i++) {
        const size_t li = its[i]->res.rt.end - its[i]->res.rt.start;
        if (li > len) len = li;
        n_batch_samples += li;
    }
    n_batches++;
    n_batch_slot_samples += (unsigned long long)len * (unsigned long long)(16 * ((nmax + 15) / 16));
    for (int i = 0; i < n; i += 16) {
        size_t lt = 0;
        for (int k = i; k < n && k < i + 16; k++) { const size_t lk = its[k]->res.rt.end - its[k]->res.rt.start; if (lk > lt) lt = lk; }
        n_tile_slot_samples += 16ull * lt;
    }
    double t0 = now_s();
    int nslot = n;
    pb.b = acquire_batch(eng, mdl, n, len, slot, &pb.cached, &nslot);
    (void)nslot;
    t_phase[2] += now_s() - t0; t0 = now_s();
    const unsigned flags = run_flags();
    int rc_sub = (NULL == pb.b) ? -1 : ffhip_batch_set_prepared(pb.b, prep, pb.idx);
    t_phase[6] += now_s() - t0;
    const double t1 = now_s();
    if (0 == rc_sub) rc_sub = batch_run(pb.b, flags, pb.its, n);
    t_phase[7] += now_s() - t1;
    if (0 != rc_sub) {
        warnx("%s", ffhip_last_error());
        if (pb.b && !pb.cached) ffhip_batch_destroy(pb.b);
        pb.b = NULL;
    }
    t_phase[3] += now_s() - t0;
    return pb;
}

static int by_length_desc(const void *x, const void *y);
static void collect_batch(const struct ffhip_model *mdl, pending_batch *pb);
/* A packed batch that failed, at submit or at collect: its reads are called again one read a row, here and now, in batch objects of their own (the cached ones
 * may be in flight) -- no read is dropped for it.  Rare by construction (the engine itself re-runs a batch whose layer launch timed out): written for clarity. */
static void call_one_read_a_row(const struct ffhip_model *mdl, const pending_batch *failed) {
    item **its = failed->its;
    const int n = failed->n;
    warnx("a packed batch of %d read(s) failed; its reads go to one-read-a-row batches", n);
    qsort(its, n, sizeof(item *), by_length_desc);
    for (int i = 0; i < n; ) {
        const size_t longest = its[i]->res.rt.end - its[i]->res.rt.start;
        int g = 1;
        while (i + g < n && g < args.batch && 4 * (its[i + g]->res.rt.end - its[i + g]->res.rt.start) >= 3 * longest) g++;
        pending_batch one = { NULL, 0, g, malloc(g * sizeof(int)), malloc(g * sizeof(item *)), failed->prep, NULL, 0 };
        if (one.idx && one.its) {
            memcpy(one.its, its + i, g * sizeof(item *));
            for (int k = 0; k < g; k++) one.idx[k] = its[i + k]->prepared;
            one.b = ffhip_batch_create(flappie_hip_engine(), mdl, g, longest);
            int rc = (NULL == one.b) ? -1 : ffhip_batch_set_prepared(one.b, failed->prep, one.idx);
            if (0 == rc) rc = batch_run(one.b, run_flags(), one.its, g);
            if (0 != rc) { warnx("%s", ffhip_last_error()); if (one.b) ffhip_batch_destroy(one.b); one.b = NULL; }
        }
        collect_batch(mdl, &one);                      /* (a failure there counts the group's reads as not called) */
        i += g;
    }
}

static void collect_batch(const struct ffhip_model *mdl, pending_batch *pb) {
    ffhip_batch *b = pb->b;
    item **its = pb->its;
    const int n = pb->n, cached = pb->cached, *idx = pb->idx;
    const ffhip_prep *prep = pb->prep;
    double t0 = now_s();
    if (NULL == b || 0 != ffhip_batch_finish(b)) {
        if (b) { warnx("%s", ffhip_last_error()); if (!cached) ffhip_batch_destroy(b); }
        if (pb->packed && its) call_one_read_a_row(mdl, pb);
        else n_lost_reads += (unsigned long long)n;
        free(pb->idx); free(pb->its);
        pb->b = NULL;
        return;
    }
    t_phase[3] += now_s() - t0; t0 = now_s();
    const size_t nblock_cap = ffhip_batch_nblock(b), nstate = 2 * ffhip_model_nbase(mdl);
    (void)nblock_cap; (void)nstate;
#ifdef BUILD_RUNNIE
    if (args.fasta) {   /* the reads' runs and run-length estimates came down with the batch (k_rle_runs); each run's base expanded `est` times, 60 a line */
        for (int i = 0; i < n; i++) {
            ffhip_rle_runs rr;
            if (0 != ffhip_batch_rle_runs(b, i, &rr)) { warnx("%s", ffhip_last_error()); continue; }
            char *text = NULL;
            if (args.rlc || (rr.nrun > 0 && !rr.failed)) {
                const size_t len = args.rlc ? rr.nrun : (size_t)rr.length;
                char *seq = malloc(len + 1);
                text = malloc(len + len / 60 + 2);
                if (NULL == seq || NULL == text) { free(seq); free(text); warnx("out of memory for a sequence of %zu bases", len); continue; }
                size_t o = 0;
                for (size_t k = 0; k < rr.nrun; k++) {
                    const size_t cnt = args.rlc ? 1 : (size_t)rr.est[k];
                    memset(seq + o, basechar(rr.base[k]), cnt);
                    o += cnt;
                }
                size_t t = 0;
                for (size_t st = 0; st < len; st += 60) {
                    const size_t w = (len - st < 60) ? len - st : 60;
                    if (st) text[t++] = '\n';
                    memcpy(text + t, seq + st, w);
                    t += w;
                }
                text[t++] = '\n';
                text[t] = 0;
                free(seq);
            }
            its[i]->rle_text = text;
            its[i]->rle_nocall = (NULL == text);
            n_called_reads++;
            n_called_samples += its[i]->res.rt.end - its[i]->res.rt.start;
            n_raw_samples += its[i]->res.rt.n;
            its[i]->res.score = ffhip_batch_score(b, i);
            its[i]->res.nblock = ffhip_batch_read_nblock(b, i);
        }
        t_phase[4] += now_s() - t0; t0 = now_s();
        if (!cached) ffhip_batch_destroy(b);
        t_phase[2] += now_s() - t0;
        free(pb->idx); free(pb->its);
        pb->b = NULL;
        return;
    } else {   /* runnie.c:262-313: path from decode_crf_runlength, then one line per emitted base with the discrete-Weibull
         * shape and scale of the block that emitted it and the dwell in blocks */
        const size_t nbase = ffhip_model_nbase(mdl), P = ffhip_model_nparam(mdl);
        int *path = malloc((nblock_cap + 1) * sizeof(int));
        float *qp = malloc((nblock_cap + 1) * sizeof(float)), *mat = malloc(nblock_cap * P * sizeof(float));
        for (int i = 0; path && qp && mat && i < n; i++) {
            const size_t nblock = ffhip_batch_read_nblock(b, i);
            if (0 != ffhip_batch_get_path(b, i, path, qp)) continue;
            if (0 != (args.viterbi_only ? ffhip_batch_get_transitions(b, i, mat) : ffhip_batch_get_posterior(b, i, mat))) continue;
            size_t cap = 64 * (nblock + 1), len = 0;
            char *text = malloc(cap);
            if (NULL == text) continue;
            text[0] = 0;
            int dwell = 1, last_blk = -1;
            for (size_t blk = 0; blk <= nblock; blk++) {
                const int emit = (blk < nblock) ? (path[blk] < (int)nbase) : 1;      /* the final pass flushes the last run */
                if (!emit) { dwell += 1; continue; }
                if (last_blk >= 0) {
                    const int base = path[last_blk];
                    /* %f of a huge value prints ~47 characters: grow the buffer instead of trusting the 64-per-block estimate
                     * (snprintf returns the would-be length, so an unchecked `len +=` walks past `cap` after one truncation) */
                    for (;;) {
                        const int ret = snprintf(text + len, cap - len, "%c\t%f\t%f\t%d\n", basechar(base), mat[(size_t)last_blk * P + base],
                                                 mat[(size_t)last_blk * P + nbase + base], dwell);
                        if (ret >= 0 && (size_t)ret < cap - len) { len += (size_t)ret; break; }
                        char *bigger = (ret < 0) ? NULL : realloc(text, 2 * cap + (size_t)ret);
                        if (NULL == bigger) { text[len] = 0; blk = nblock; break; }      /* out of memory: keep what fits */
                        text = bigger;
                        cap = 2 * cap + (size_t)ret;
                    }
                }
                last_blk = (int)blk;
                dwell = 1;
            }
            its[i]->rle_text = text;
            n_called_reads++;                                  /* (FLAPPIE_CLI_TIMING's "basecalled:" line) */
            n_called_samples += its[i]->res.rt.end - its[i]->res.rt.start;
            n_raw_samples += its[i]->res.rt.n;
            its[i]->res.score = ffhip_batch_score(b, i);
            its[i]->res.nblock = nblock;
        }
        free(path); free(qp); free(mat);
        t_phase[4] += now_s() - t0; t0 = now_s();
        if (!cached) ffhip_batch_destroy(b);
        t_phase[2] += now_s() - t0;
        free(pb->idx); free(pb->its);
        pb->b = NULL;
        return;
    }
#endif
    for (int i = 0; i < n; i++) {
        struct _raw_basecall_info *r = &its[i]->res;
        const size_t nblock = ffhip_batch_read_nblock(b, i);
        n_called_reads++;
        n_called_samples += r->rt.end - r->rt.start;
        n_raw_samples += r->rt.n;
        size_t blen = 0;
        const char *bases = ffhip_batch_basecall(b, i, &blen);
        r->basecall = strdup(bases);
        r->quality = strdup(ffhip_batch_quality(b, i));
        r->basecall_length = blen;
        r->score = ffhip_batch_score(b, i);
        r->nblock = nblock;
        r->pos = calloc(nblock + 1, sizeof(int));
        if (args.modbase_tags) {
            const uint8_t *ml = NULL;
            size_t mlen = 0;
            if (0 != ffhip_batch_mod_probs(b, i, &ml, &mlen) || mlen != blen) warnx("%s", ffhip_last_error());
            else if (NULL != (its[i]->ml = malloc(blen ? blen : 1))) memcpy(its[i]->ml, ml, blen);
        }
        if (args.emit_moves) {                                 /* the move table stays in signal order whatever --reverse does to the strings */
            const uint8_t *mv = NULL;
            size_t nmv = 0;
            if (0 != ffhip_batch_moves(b, i, &mv, &nmv) || nmv != nblock) warnx("%s", ffhip_last_error());
            else if (NULL != (its[i]->mv = malloc(nblock ? nblock : 1))) {
                memcpy(its[i]->mv, mv, nblock);
                size_t k = 0;
                for (size_t blk = 0; r->pos && blk < nblock && k < blen; blk++) if (mv[blk]) r->pos[k++] = (int)blk;      /* the block of base k */
                its[i]->mv_stride = (int)ffhip_model_stride(mdl);
                its[i]->sm = its[i]->sd = 0.0f;
                if (args.delta == 0.0f && 0 != ffhip_prep_stats(prep, idx[i], &its[i]->sm, &its[i]->sd)) warnx("%s", ffhip_last_error());
            }
        }
        if (bc_dev) {                                          /* the record describes the call in signal order whatever --reverse does to the strings */
            if (0 != ffhip_batch_barcode(b, i, &its[i]->bc) || its[i]->bc.best >= bc_kit->n) warnx("%s", ffhip_last_error());
            else { its[i]->have_bc = 1; bc_count[its[i]->bc.best >= 0 ? its[i]->bc.best : bc_kit->n]++; }
        }
        if (ad_dev) {                                          /* likewise */
            const ffhip_adapter_hit *hits = NULL;
            if (0 != ffhip_batch_adapters(b, i, &its[i]->ad_head, &hits)) warnx("%s", ffhip_last_error());
            else if (its[i]->ad_head.kept < 0 || its[i]->ad_head.kept > FFHIP_ADAPTER_MAX_HITS) warnx("A bad adapter record for %s", its[i]->filename);
            else {
                memcpy(its[i]->ad_hits, hits, sizeof its[i]->ad_hits);
                its[i]->have_ad = 1;
                for (int h = 0; h < its[i]->ad_head.kept; h++) {
                    if (hits[h].pattern < 0 || hits[h].pattern >= ad_kit->n) { its[i]->have_ad = 0; break; }
                    ad_count[hits[h].pattern]++;
                }
                if (its[i]->have_ad && its[i]->ad_head.nhit > 0) ad_reads_with_hit++;
            }
        }
        if (mp_dev) {                                          /* likewise: the whole call in signal order */
            if (0 != ffhip_batch_map(b, i, &its[i]->mp)) warnx("%s", ffhip_last_error());
            else its[i]->have_mp = 1;
        }
        if (pt_on) {                                           /* likewise */
            if (0 != ffhip_batch_polytail(b, i, &its[i]->pt)) warnx("%s", ffhip_last_error());
            else { its[i]->have_pt = 1; if (0 != flappie_polytail_count(&pt_sum, &its[i]->pt)) warnx("out of memory for the poly tail summary"); }
        }
        if ((rm_refs && its[i]->rm_ref >= 0) || rfm_on) {      /* the read's mapping to its sequence: the table's line is written with the read's record */
            ffhip_remap_call rc;
            if (0 != ffhip_batch_remap(b, i, &rc)) warnx("%s", ffhip_last_error());
            else {
                its[i]->have_rm = 1; its[i]->rm_status = rc.status; its[i]->rm_L = rc.L; its[i]->rm_nblock = rc.nblock; its[i]->rm_score = rc.score;
                if (1 == rc.status && NULL != (its[i]->rm = malloc(rc.nblock ? rc.nblock : 1))) memcpy(its[i]->rm, rc.rm, rc.nblock);
                its[i]->mv_stride = (int)ffhip_model_stride(mdl);
                if (ev_out && 1 == rc.status) {                /* ... and the signal under its bases */
                    const ffhip_event *ev = NULL;
                    size_t nev = 0;
                    if (0 != ffhip_batch_events(b, i, &ev, &nev) || NULL == ev || nev != rc.L) warnx("No events returned for %s: %s", its[i]->filename, ffhip_last_error());
                    else if (NULL != (its[i]->ev = malloc(nev * sizeof(ffhip_event)))) memcpy(its[i]->ev, ev, nev * sizeof(ffhip_event));
                }
                if (md_out && 1 == rc.status) {                /* ... and the scores at its C positions */
                    const ffhip_site_mod *sm = NULL;
                    size_t nsm = 0;
                    if (0 != ffhip_batch_site_mods(b, i, &sm, &nsm) || NULL == sm) warnx("No site mods returned for %s: %s", its[i]->filename, ffhip_last_error());
                    else if (NULL != (its[i]->smods = malloc((nsm ? nsm : 1) * sizeof(ffhip_site_mod)))) { memcpy(its[i]->smods, sm, nsm * sizeof(ffhip_site_mod)); its[i]->nsmods = nsm; }
                }
                if (vr_out && 1 == rc.status) {                /* ... and the scores of its variants */
                    const ffhip_variant_call *vc = NULL;
                    size_t nvc = 0;
                    if (0 != ffhip_batch_variant_calls(b, i, &vc, &nvc) || NULL == vc) warnx("No variant calls returned for %s: %s", its[i]->filename, ffhip_last_error());
                    else if (NULL != (its[i]->vcalls = malloc((nvc ? nvc : 1) * sizeof(ffhip_variant_call)))) { memcpy(its[i]->vcalls, vc, nvc * sizeof(ffhip_variant_call)); its[i]->nvcalls = nvc; }
                }
            }
        }
        if ((tr_refs && its[i]->tr_ref >= 0) || tfm_on) {      /* the call against its truth, in signal order whatever --reverse does below */
            ffhip_truth_call tc;
            if (0 != ffhip_batch_truth(b, i, &tc)) warnx("%s", ffhip_last_error());
            else {
                its[i]->have_tr = 1;
                its[i]->tr = (flappie_truth_rec){ tc.status, tc.n, tc.m, args.truth_band, tc.maxdev, tc.dist, tc.n_match, tc.n_mismatch, tc.n_ins, tc.n_del };
                its[i]->tr_nops = 0;
                if (1 == tc.status && NULL != (its[i]->tr_ops = malloc(tc.nops ? tc.nops : 1))) { memcpy(its[i]->tr_ops, tc.ops, tc.nops); its[i]->tr_nops = tc.nops; }
            }
        }
        if (args.reverse) {                                    /* flappie.c:294-297 */
            reverse_char_array(r->basecall, blen);
            reverse_char_array(r->quality, blen);
            for (size_t k = 0; its[i]->ml && k < blen / 2; k++) { const uint8_t t = its[i]->ml[k]; its[i]->ml[k] = its[i]->ml[blen - 1 - k]; its[i]->ml[blen - 1 - k] = t; }
        }
        if (args.trace) {
            int32_t *tmp = malloc((nblock + 1) * nstate * sizeof(int32_t));
            r->trace = make_flappie_imatrix(nstate, nblock + 1);
            if (tmp && r->trace && 0 == ffhip_batch_get_trace(b, i, tmp)) {
                for (size_t c = 0; c <= nblock; c++) memcpy(r->trace->data.f + c * r->trace->stride, tmp + c * nstate, nstate * sizeof(int32_t));
            } else {
                r->trace = free_flappie_imatrix(r->trace);
            }
            free(tmp);
            /* write_summary stores the signal the network saw (fast5_interface.c:332-335) */
            if (NULL == r->rt.raw) r->rt.raw = calloc(r->rt.n ? r->rt.n : 1, sizeof(float));      /* (a read that came as DAC values has no float array yet) */
            if (NULL == r->rt.raw || 0 != ffhip_prep_get_signal(prep, idx[i], r->rt.raw + r->rt.start)) warnx("%s", NULL == r->rt.raw ? "out of memory" : ffhip_last_error());
        }
    }
    t_phase[4] += now_s() - t0; t0 = now_s();
    if (!cached) ffhip_batch_destroy(b);
    t_phase[2] += now_s() - t0;
    free(pb->idx); free(pb->its);
    pb->b = NULL;
}

/* A chunk of reads on its way through the GPU: prepared in one device pass (flappie.c:248-262: trim/segment, then med-MAD or
 * --delta), cut into batches of similar trimmed length, written in input order (flappie.c:371-384).  The batch pipeline does
 * NOT drain between chunks: the first batch of chunk k+1 is submitted before the last batch of chunk k is collected, and chunk
 * k is written while chunk k+1 runs -- the signal preparation of k+1 and the output of k overlap GPU work. */
typedef struct chunk_ctx {
    item *items;
    int n, buf;                  /* buf: which of the reader's buffers holds the items (released when the chunk is written) */
    ffhip_prep *prep;
    raw_table *rts;
    ffhip_dac_read *dacs;        /* a chunk of DAC reads (read_chunk cuts a chunk where the kind changes: it holds one kind) */
    item **group;
    int m2, submitted, collected, all_submitted, live;
} chunk_ctx;

static int by_length_desc(const void *x, const void *y) {
    const item *a = *(item *const *)x, *b = *(item *const *)y;
    const size_t la = a->res.rt.end - a->res.rt.start, lb = b->res.rt.end - b->res.rt.start;
    return (la < lb) - (la > lb);
}

/* The chunk's device pass in two halves (round 6, third session): begin enqueues it (wait = 0: ffhip_prep_begin returns at once), finish waits for it, takes the
 * ranges and sorts the reads.  pipe_chunk begins chunk k + 1 before it submits chunk k's batches when that chunk is a large one: its preparation -- one workgroup a
 * read, as long as the longest read's selection passes last, and held behind the engine's last layer launch -- then runs beside chunk k's convolutions instead of in
 * front of chunk k + 1's (profiles/r06_pack_trace.txt). */
static void chunk_begin(struct ffhip_engine *eng, chunk_ctx *c, item *items, int n, int buf, int wait) {
    memset(c, 0, sizeof(*c));
    c->items = items; c->n = n; c->buf = buf; c->live = 1;
    c->group = calloc(n > 0 ? n : 1, sizeof(item *));
    c->rts = calloc(n > 0 ? n : 1, sizeof(raw_table));
    c->dacs = calloc(n > 0 ? n : 1, sizeof(ffhip_dac_read));
    int m = 0, ndac = 0;
    for (int i = 0; i < n; i++) {
        items[i].prepared = -1;
        if (!item_has_signal(&items[i])) continue;
        if (NULL != items[i].dac) { c->dacs[m] = (ffhip_dac_read){ items[i].dac, items[i].res.rt.n, items[i].dac_offset, items[i].dac_unit }; ndac++; }
        else c->rts[m] = items[i].res.rt;
        items[i].prepared = m++;
    }
    if (ndac > 0 && ndac < m) errx(EXIT_FAILURE, "internal error: a chunk holds DAC reads and float reads");
    double tp0 = now_s();
    const int pmode = (args.delta == 0.0f) ? FFHIP_PREP_MEDMAD : FFHIP_PREP_DELTA;
    if (m > 0 && ndac > 0) c->prep = (wait ? ffhip_prep_create_dac : ffhip_prep_begin_dac)(eng, c->dacs, m, args.trim_start, args.trim_end, args.varseg_chunk, args.varseg_thresh, pmode, args.delta);
    else c->prep = (m > 0) ? (wait ? ffhip_prep_create : ffhip_prep_begin)(eng, c->rts, m, args.trim_start, args.trim_end, args.varseg_chunk, args.varseg_thresh, pmode, args.delta) : NULL;
    t_phase[1] += now_s() - tp0;
    if (m > 0 && NULL == c->prep) warnx("%s", ffhip_last_error());
}

static void chunk_begin_finish(chunk_ctx *c) {
    item *items = c->items;
    const int n = c->n;
    double tp0 = now_s();
    if (NULL != c->prep && 0 != ffhip_prep_finish(c->prep)) { warnx("%s", ffhip_last_error()); ffhip_prep_destroy(c->prep); c->prep = NULL; }
    t_phase[1] += now_s() - tp0;
    for (int i = 0; i < n; i++) {
        if (items[i].prepared < 0) continue;
        size_t st = 0, en = 0;
        if (NULL == c->prep || 0 != ffhip_prep_range(c->prep, items[i].prepared, &st, &en) || st >= en) { items[i].prepared = -1; continue; }
        items[i].res.rt.start = st;
        items[i].res.rt.end = en;
    }
    /* ragged batches: reads sorted by trimmed length, a batch takes up to --batch consecutive ones as long as the
     * shortest is at least 3/4 of the longest (a read tile of 16 costs what its longest read costs) */
    for (int i = 0; i < n; i++) if (items[i].prepared >= 0) c->group[c->m2++] = &items[i];
    qsort(c->group, c->m2, sizeof(item *), by_length_desc);
}

/* --trace: the filters of the summary file (shuffle + deflate, 10-15 ms per 100 000-sample read) are the one expensive step of
 * the output side and libhdf5 runs them under its caller's lock; here they run in worker threads, per read, outside libhdf5
 * (summary_pack_create), and the writer below only hands finished chunks over */
typedef struct { chunk_ctx *c; summary_pack **packs; int k, nthread; } pack_job;
static void *pack_worker(void *arg) {
    pack_job *j = arg;
    for (int i = j->k; i < j->c->n; i += j->nthread) {
        item *it = &j->c->items[i];
        if (NULL != it->res.basecall) j->packs[i] = summary_pack_create(it->res, args.compression_chunk_size, args.compression_level);
    }
    return NULL;
}
static summary_pack **pack_chunk(chunk_ctx *c) {
    summary_pack **packs = calloc(c->n > 0 ? c->n : 1, sizeof(*packs));
    if (NULL == packs) return NULL;
    const char *e = getenv("FLAPPIE_TRACE_THREADS");
    int nthread = e ? atoi(e) : 16;
    if (nthread < 1) nthread = 1;
    if (nthread > 64) nthread = 64;
    if (nthread > c->n) nthread = c->n > 0 ? c->n : 1;
    pthread_t th[64];
    pack_job jobs[64];
    char started[64];
    for (int k = 0; k < nthread; k++) {                       /* the last share runs here; so does any share whose thread did not start */
        jobs[k] = (pack_job){ c, packs, k, nthread };
        started[k] = (k + 1 < nthread) && 0 == pthread_create(&th[k], NULL, pack_worker, &jobs[k]);
        if (!started[k]) pack_worker(&jobs[k]);
    }
    for (int k = 0; k < nthread; k++) if (started[k]) pthread_join(th[k], NULL);
    return packs;
}

/* output of a finished chunk, in input order; releases what the chunk owns */
static void chunk_finish(chunk_ctx *c, hid_t hdf5out) {
    const double to0 = now_s();
    summary_pack **packs = (hdf5out >= 0) ? pack_chunk(c) : NULL;
    for (int i = 0; i < c->n; i++) {
        item *it = &c->items[i];
#ifdef BUILD_RUNNIE
        if (args.fasta && it->rle_nocall) {
            fprintf(stderr, "No basecall returned for %s\n", it->res.rt.uuid ? it->res.rt.uuid : "");      /* (decode_runnie.py's words, its read name) */
        } else if (NULL != it->rle_text && args.fasta) {
            fprintf(args.output, ">%s\n%s", it->res.rt.uuid ? it->res.rt.uuid : "", it->rle_text);
            free(it->rle_text);
            it->rle_text = NULL;
        } else if (NULL != it->rle_text) {
            fprintf(args.output, "# %s\n%s", it->res.rt.uuid ? it->res.rt.uuid : "", it->rle_text);      /* runnie.c:280 */
            free(it->rle_text);
            it->rle_text = NULL;
        } else {
            warnx("No basecall returned for %s", it->filename);
        }
        it->rle_nocall = 0;
        free_raw_basecall_info(&it->res);
        free(it->dac);
        it->dac = NULL;
        free(it->filename);
        continue;
#endif
        if (NULL == it->res.basecall) {
            warnx("No basecall returned for %s", it->filename);
        } else {
            char *fn = strdup(it->filename);
            const char *base = basename(fn);
            const char *uuid = it->res.rt.uuid ? it->res.rt.uuid : "";
            char *multi_name = NULL;              /* --no-uuid, a read of a multi-read file: <file>:<read id> (the file's name alone would stand for thousands of reads) */
            if (it->from_multi && NULL != (multi_name = malloc(strlen(base) + strlen(uuid) + 2))) { sprintf(multi_name, "%s:%s", base, uuid); base = multi_name; }
            /* --modbase-tags: Z is written as C here, in the record only -- the trace file below keeps the call as it is */
            if (pt_on) {                             /* every tag the other options bring, and the poly tail tags behind them */
                const flappie_adapter_out ad = { &it->ad_head, it->ad_hits, ad_kit, ad_trim, ad_split, ad_window, (size_t)ad_min_length };
                if (!it->have_pt) warnx("No poly tail record for %s", it->filename);
                else if (NULL != ad_kit && !it->have_ad) warnx("No adapter record for %s", it->filename);
                else if (NULL != bc_kit && !it->have_bc) warnx("No barcode record for %s", it->filename);
                else if (args.emit_moves && NULL == it->mv) warnx("No move table for %s", it->filename);
                else if (args.modbase_tags && NULL == it->ml) warnx("No base-modification probabilities for %s", it->filename);
                else fprintf_polytail_record(args.outformat, args.output, uuid, base, args.uuid, args.prefix, it->res, args.modbase_tags ? it->ml : NULL,
                                             args.emit_moves ? it->mv : NULL, it->mv_stride, it->sm, it->sd, args.delta != 0.0f, bc_kit ? &it->bc : NULL, bc_kit,
                                             args.bc_trim, ad_kit ? &ad : NULL, args.reverse, ad_stats, &it->pt);
            } else if (NULL != ad_kit) {
                const flappie_adapter_out ad = { &it->ad_head, it->ad_hits, ad_kit, ad_trim, ad_split, ad_window, (size_t)ad_min_length };
                if (!it->have_ad) warnx("No adapter record for %s", it->filename);
                else if (NULL != bc_kit && !it->have_bc) warnx("No barcode record for %s", it->filename);
                else if (args.emit_moves && NULL == it->mv) warnx("No move table for %s", it->filename);
                else if (args.modbase_tags && NULL == it->ml) warnx("No base-modification probabilities for %s", it->filename);
                else fprintf_adapter_record(args.outformat, args.output, uuid, base, args.uuid, args.prefix, it->res, args.modbase_tags ? it->ml : NULL,
                                            args.emit_moves ? it->mv : NULL, it->mv_stride, it->sm, it->sd, args.delta != 0.0f, bc_kit ? &it->bc : NULL, bc_kit,
                                            args.bc_trim, &ad, args.reverse, ad_stats);
            } else if (NULL != bc_kit) {
                if (!it->have_bc) warnx("No barcode record for %s", it->filename);
                else if (args.emit_moves && NULL == it->mv) warnx("No move table for %s", it->filename);
                else if (args.modbase_tags && NULL == it->ml) warnx("No base-modification probabilities for %s", it->filename);
                else fprintf_barcode_record(args.outformat, args.output, uuid, base, args.uuid, args.prefix, it->res, args.modbase_tags ? it->ml : NULL,
                                            args.emit_moves ? it->mv : NULL, it->mv_stride, it->sm, it->sd, args.delta != 0.0f, &it->bc, bc_kit, args.bc_trim, args.reverse);
            } else if (args.emit_moves) {
                if (NULL == it->mv) warnx("No move table for %s", it->filename);
                else if (args.modbase_tags && NULL == it->ml) warnx("No base-modification probabilities for %s", it->filename);
                else fprintf_moves_record(args.outformat, args.output, uuid, base, args.uuid, args.prefix, it->res, args.modbase_tags ? it->ml : NULL, it->mv,
                                          it->mv_stride, it->sm, it->sd, args.delta != 0.0f);
            } else if (args.modbase_tags) {
                if (it->ml) fprintf_modbase_record(args.outformat, args.output, uuid, base, args.uuid, args.prefix, it->res, it->ml);
                else warnx("No base-modification probabilities for %s", it->filename);
            } else {
                fprintf_format(args.outformat, args.output, uuid, base, args.uuid, args.prefix, it->res);
            }
            if (rm_refs) {                                     /* stdout above is what it is without --remap; the table gets the read's line */
                if (it->rm_ref < 0) rm_count[1]++;
                else if (!it->have_rm) warnx("No mapping returned for %s", it->filename);
                else {
                    const size_t L = rm_refs->bad[it->rm_ref] ? 0 : rm_refs->len[it->rm_ref];
                    const long dev = flappie_remap_write_line(rm_out, rm_refs->name[it->rm_ref], it->rm_status, it->rm_nblock, it->mv_stride, it->res.rt.start, L,
                                                              args.remap_band, it->rm, it->rm_score);
                    if (dev < 0) warnx("The moves of %s do not fit its sequence", it->filename);
                    if (1 == it->rm_status) { rm_count[0]++; if (dev == (long)args.remap_band) rm_count[3]++; } else rm_count[2]++;
                    if (ev_out && 1 == it->rm_status) {
                        if (NULL == it->ev || it->rm_L != L) warnx("No events for %s", it->filename);
                        else {
                            write_events(ev_out, rm_refs->name[it->rm_ref], rm_refs->codes[it->rm_ref], "ACGTZ", it->res.rt.start, it->ev, L);
                            ev_count[0]++; ev_count[1] += L;
                        }
                    }
                    if (md_out && 1 == it->rm_status) {
                        if (NULL == it->smods || it->rm_L != L) warnx("No site mods for %s", it->filename);
                        else if (0 != flappie_sitemods_write(md_out, rm_refs->name[it->rm_ref], rm_refs->codes[it->rm_ref], L, "ACGTZ", it->smods, it->nsmods))
                            warnx("The site mods of %s do not fit its sequence", it->filename);
                        else { md_count[0]++; md_count[1] += it->nsmods; }
                    }
                    if (vr_out && 1 == it->rm_status) {
                        const size_t nv = flappie_variants_of(vr_vars, it->rm_ref, NULL);
                        ffhip_variant *var = malloc((nv ? nv : 1) * sizeof *var);
                        if (NULL == it->vcalls || it->nvcalls != nv || it->rm_L != L || NULL == var) warnx("No variant calls for %s", it->filename);
                        else if (flappie_variants_of(vr_vars, it->rm_ref, var), 0 != flappie_variants_write(vr_out, rm_refs->name[it->rm_ref], rm_refs->codes[it->rm_ref], L,
                                                                                                              "ACGTZ", var, it->vcalls, nv))
                            warnx("The variant calls of %s do not fit its sequence", it->filename);
                        else if (nv) { vr_count[0]++; vr_count[1] += nv; vr_done[it->rm_ref] = 1; }
                        free(var);
                    }
                }
            }
            if (rfm_on) {                                      /* --remap-from-map: a line a mapped read, with its place behind the mapping; its events */
                const char *name = *uuid ? uuid : base;       /* (hits.tsv's name) */
                int k = 0;
                char o = '+';
                long a = 0, e = 0;
                if (!it->have_mp || !it->have_rm) warnx("No %s returned for %s", it->have_mp ? "mapping" : "map record", it->filename);
                if (!it->have_mp || 1 != it->mp.status || !it->have_rm) rm_count[1]++;
                else if (0 != flappie_map_forward(mp_ref, it->mp.q, it->mp.tstart, it->mp.tend, &k, &o, &a, &e)) warnx("The map record of %s does not fit the reference", it->filename);
                else {
                    const size_t L = (size_t)(e - a);
                    const long dev = (1 == it->rm_status && it->rm_L != L) ? -1 :
                        flappie_remap_write_placed_line(rm_out, name, it->rm_status, it->rm_nblock, it->mv_stride, it->res.rt.start, L, args.remap_band, it->rm, it->rm_score,
                                                        mp_ref->name[k], o, a, e);
                    if (dev < 0) warnx("The moves of %s do not fit its stretch of the reference", it->filename);
                    if (1 == it->rm_status) { rm_count[0]++; if (dev == (long)args.remap_band) rm_count[3]++; } else rm_count[2]++;
                    if (ev_out && 1 == it->rm_status && dev >= 0) {
                        uint8_t *codes = malloc(L ? L : 1);  /* the stretch in signal order, from the letters --map-records writes */
                        if (NULL == it->ev || NULL == codes) warnx("No events for %s", it->filename);
                        else {
                            const char *sq = mp_ref->seq[k];
                            for (size_t i = 0; i < L; i++) { const int c = (int)(strchr("ACGT", '+' == o ? sq[a + (long)i] : sq[e - 1 - (long)i]) - "ACGT"); codes[i] = (uint8_t)('+' == o ? c : 3 - c); }
                            write_events(ev_out, name, codes, "ACGTZ", it->res.rt.start, it->ev, L);
                            ev_count[0]++; ev_count[1] += L;
                        }
                        free(codes);
                    }
                }
            }
            if (mp_ref) {                                      /* likewise for --map: a line a read, and the mapped read's own stretch */
                const char *name = *uuid ? uuid : base;       /* (what --truth and --remap find a record by) */
                if (!it->have_mp) warnx("No map record returned for %s", it->filename);
                else if (0 != flappie_map_write_line(mp_out, name, &it->mp, mp_ref)) warnx("The map record of %s does not fit the reference", it->filename);
                else {
                    flappie_map_summary_add(&mp_sum, &it->mp, map_window);
                    if (mp_recs && flappie_map_write_record(mp_recs, name, &it->mp, mp_ref) < 0) warnx("The span of %s does not fit the reference", it->filename);
                }
            }
            if (tr_refs) {                                     /* likewise for --truth */
                if (it->tr_ref < 0) flappie_truth_summary_add(&tr_sum, NULL);
                else if (!it->have_tr) warnx("No alignment returned for %s", it->filename);
                else {
                    if (0 != flappie_truth_write_line(tr_out, tr_refs->name[it->tr_ref], &it->tr, it->tr_ops, it->tr_nops)) warnx("The ops of %s do not fit its record", it->filename);
                    if (0 != flappie_truth_summary_add(&tr_sum, &it->tr)) warnx("--truth: out of memory for the summary");
                }
            }
            if (tfm_on) {                                      /* --truth-from-map: a line a mapped read, with its place behind the alignment; the SAM file */
                const char *name = *uuid ? uuid : base;       /* (hits.tsv's name) */
                const int mapped = it->have_mp && 1 == it->mp.status;
                if (!it->have_mp || !it->have_tr) warnx("No %s returned for %s", it->have_mp ? "alignment" : "map record", it->filename);
                if (!mapped || !it->have_tr) flappie_truth_summary_add(&tr_sum, NULL);
                else {
                    if (0 != flappie_align_write_acc_line(tr_out, name, &it->tr, it->tr_ops, it->tr_nops, &it->mp, mp_ref)) warnx("The ops of %s do not fit its record", it->filename);
                    if (0 != flappie_truth_summary_add(&tr_sum, &it->tr)) warnx("--truth-from-map: out of memory for the summary");
                }
                if (tfm_sam) {                                 /* the whole call in signal order, whatever --reverse did to the strings */
                    const size_t n = strlen(it->res.basecall);
                    char *sq = strdup(it->res.basecall), *ql = it->res.quality ? strdup(it->res.quality) : NULL;
                    if (NULL == sq || NULL == ql || strlen(ql) != n) warnx("--map-sam: no call and quality of one length for %s", it->filename);
                    else {
                        if (args.reverse) { reverse_char_array(sq, n); reverse_char_array(ql, n); }
                        if (flappie_align_write_sam_line(tfm_sam, name, sq, ql, n, (mapped && it->have_tr) ? &it->tr : NULL, it->tr_ops, it->tr_nops, &it->mp, mp_ref) < 0)
                            warnx("The alignment of %s does not fit the reference", it->filename);
                    }
                    free(sq);
                    free(ql);
                }
            }
            if (hdf5out >= 0) {
                pthread_mutex_lock(&hdf5_lock);
                if (packs && packs[i]) summary_pack_write(hdf5out, args.uuid ? uuid : base, packs[i]);
                else write_summary(hdf5out, args.uuid ? uuid : base, it->res, args.compression_chunk_size, args.compression_level);
                pthread_mutex_unlock(&hdf5_lock);
                if (packs) { summary_pack_free(packs[i]); packs[i] = NULL; }
            }
            free(fn);
            free(multi_name);
        }
        free(it->dac);
        it->dac = NULL;
        free(it->ml);
        it->ml = NULL;
        free(it->mv);
        it->mv = NULL;
        it->have_bc = 0;
        it->have_ad = 0;
        it->have_pt = 0;
        it->have_mp = 0;
        free(it->rm);
        it->rm = NULL;
        free(it->ev);
        it->ev = NULL;
        free(it->smods);
        it->smods = NULL;
        it->nsmods = 0;
        free(it->vcalls);
        it->vcalls = NULL;
        it->nvcalls = 0;
        it->have_rm = 0;
        it->rm_ref = -1;
        free(it->tr_ops);
        it->tr_ops = NULL;
        it->have_tr = 0;
        it->tr_ref = -1;
        free_raw_basecall_info(&it->res);
        free(it->filename);
    }
    if (packs) { for (int i = 0; i < c->n; i++) summary_pack_free(packs[i]); free(packs); }
    t_phase[5] += now_s() - to0;
    free(c->rts);
    free(c->dacs);
    free(c->group);
    __atomic_store_n(&c->live, 0, __ATOMIC_RELEASE);
}

/* the pipeline's state: up to NINFLIGHT - 1 batches submitted and not collected (oldest first) while the next is submitted (by default
 * one: a batch runs while the next is set up); chunks finish (are written) strictly in order */
#define NCHUNKBUF 4
#define PACK_ROW_MAX ((size_t)1 << 18)      /* samples a row of a packed batch holds at most (262 144: workspace of a 512-row batch ~45 GB at 384 hidden units) */
static int rs_chunk_cap = 0;                 /* reads a chunk holds at most (= reads a packed batch must take) */
/* packed batches: models whose default path takes them (ffhip_model_packable: the flip-flop models, and runnie's run-length model), ordinary temperatures;
 * FLAPPIE_DEBUG=no_pack keeps the one-read-a-row batches */
static int pack_allowed(const struct ffhip_model *mdl) {
    static int v = -1;
    if (v < 0) v = (ffhip_model_packable(mdl) && args.temperature >= 0.2f && args.temperature <= 5.0f && !cli_dbg("no_pack")) ? 1 : 0;
    return v;
}
/* Reads are sorted by length inside a chunk and cut into batches there (a batch costs what its longest read costs): the more batches a chunk
 * holds, the narrower the spread of lengths inside one.  On 3500-5500-sample reads 8 instead of 4 takes 2-8 % off the GPU time of a run
 * (65 536 files: 4.07 -> 4.00 s at 384 hidden units, 2.51 -> 2.38 s at 256); 16 gains little more and delays the first and the last output. */
#define CHUNK_BATCHES 8
static struct {
    pending_batch fifo[NINFLIGHT - 1];
    int nfifo, slot;
    chunk_ctx ctx[NCHUNKBUF];
    long next_finish, nbegun;            /* chunk sequence numbers; chunk q lives in ctx[q % NCHUNKBUF] */
    void (*released)(int buf, void *arg);
    void *released_arg;
} pipe_state;

/* A WRITER THREAD takes the finished chunks, strictly in order: formatting, --trace compression and the HDF5 writes of chunk k run
 * while the main thread keeps submitting the batches of chunk k + 1 (with --trace on 100 000-sample reads the output side costs as
 * much time as the GPU side; done on the main thread it stood between two submissions).  chunk sequence numbers in
 * [writer.head, writer.tail) are ready to be written; FLAPPIE_DEBUG=no_writer_thread writes on the main thread. */
static struct { pthread_t th; pthread_mutex_t mu; pthread_cond_t cv; long head, tail; int started, stop; hid_t hdf5out; } writer =
    { 0, PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, 0, 0, 0, 0, -1 };

static void writer_do(long q) {
    chunk_ctx *c = &pipe_state.ctx[q % NCHUNKBUF];
    const int buf = c->buf;
    chunk_finish(c, writer.hdf5out);                  /* sets c->live = 0 */
    if (pipe_state.released) pipe_state.released(buf, pipe_state.released_arg);
}

static void *writer_main(void *arg) {
    (void)arg;
    pthread_mutex_lock(&writer.mu);
    for (;;) {
        while (writer.head == writer.tail && !writer.stop) pthread_cond_wait(&writer.cv, &writer.mu);
        if (writer.head == writer.tail) break;
        const long q = writer.head;
        pthread_mutex_unlock(&writer.mu);
        writer_do(q);
        pthread_mutex_lock(&writer.mu);
        writer.head++;
        pthread_cond_broadcast(&writer.cv);
    }
    pthread_mutex_unlock(&writer.mu);
    return NULL;
}

static void pipe_finish_ready(hid_t hdf5out) {
    while (pipe_state.next_finish < pipe_state.nbegun) {
        chunk_ctx *c = &pipe_state.ctx[pipe_state.next_finish % NCHUNKBUF];
        if (!(c->all_submitted && c->collected == c->submitted)) break;
        ffhip_prep_destroy(c->prep);                  /* (the engine's buffer pool belongs to this thread) */
        c->prep = NULL;
        writer.hdf5out = hdf5out;
        if (!writer.started && !cli_dbg("no_writer_thread")) writer.started = (0 == pthread_create(&writer.th, NULL, writer_main, NULL)) ? 1 : -1;
        if (writer.started == 1) {
            pthread_mutex_lock(&writer.mu);
            writer.tail = pipe_state.next_finish + 1;
            pthread_cond_broadcast(&writer.cv);
            pthread_mutex_unlock(&writer.mu);
        } else {
            writer_do(pipe_state.next_finish);
        }
        pipe_state.next_finish++;
    }
}

/* all chunks handed over so far are written (end of the run) */
static void writer_finish(void) {
    if (writer.started != 1) return;
    pthread_mutex_lock(&writer.mu);
    writer.stop = 1;
    pthread_cond_broadcast(&writer.cv);
    pthread_mutex_unlock(&writer.mu);
    pthread_join(writer.th, NULL);
}

/* collect the oldest batch in flight */
static void pipe_collect_oldest(const struct ffhip_model *mdl, hid_t hdf5out) {
    if (0 == pipe_state.nfifo) return;
    pending_batch old = pipe_state.fifo[0];
    for (int k = 1; k < pipe_state.nfifo; k++) pipe_state.fifo[k - 1] = pipe_state.fifo[k];
    pipe_state.nfifo--;
    chunk_ctx *owner = old.owner;
    collect_batch(mdl, &old);
    owner->collected++;
    pipe_finish_ready(hdf5out);
}
static void pipe_collect_all(const struct ffhip_model *mdl, hid_t hdf5out) {
    while (pipe_state.nfifo) pipe_collect_oldest(mdl, hdf5out);
}

/* reads sorted by trimmed length, longest first, in one-read-a-row batches: a batch takes up to --batch consecutive ones as long as the shortest is at least 3/4 of the
 * longest (a read tile of 16 costs what its longest read costs) */
static void run_groups(struct ffhip_engine *eng, const struct ffhip_model *mdl, struct chunk_ctx *c, item **group, int m2, hid_t hdf5out, int depth);
static int pack_failed = 0;                  /* a packed batch object could not be created (memory): the rest of the run goes one read a row */

/* the context of the next chunk to begin (chunk sequence number nbegun): its slot's previous chunk may still be with the writer */
static chunk_ctx *chunk_slot(void) {
    chunk_ctx *c = &pipe_state.ctx[pipe_state.nbegun % NCHUNKBUF];
    if (writer.started == 1) {
        pthread_mutex_lock(&writer.mu);
        while (__atomic_load_n(&c->live, __ATOMIC_ACQUIRE)) pthread_cond_wait(&writer.cv, &writer.mu);
        pthread_mutex_unlock(&writer.mu);
    }
    if (c->live) errx(EXIT_FAILURE, "internal error: chunk slot still in use");
    return c;
}
static chunk_ctx *chunk_ahead = NULL;        /* the chunk whose device pass was begun while its predecessor was handled (its items are the next pipe_chunk's) */

/* look_ahead (may be NULL): asked AFTER this chunk's own device pass has been waited for -- i.e. when the batch in flight has just ended -- whether the chunk that follows is in
 * the reader's buffers already and is a large one; its device pass is then begun here, in front of this chunk's batches, and runs beside their convolutions */
typedef int (*look_ahead_fn)(item **items, int *n, int *buf);
static void pipe_chunk(struct ffhip_engine *eng, const struct ffhip_model *mdl, item *items, int n, int buf, hid_t hdf5out, look_ahead_fn look_ahead) {
    chunk_ctx *c = chunk_ahead;
    if (NULL != c) {
        if (c->items != items || c->n != n) errx(EXIT_FAILURE, "internal error: the chunk prepared ahead is not the one that follows");
        chunk_ahead = NULL;
    } else {
        c = chunk_slot();
        chunk_begin(eng, c, items, n, buf, 1);     /* the device pass runs beside the batch still in flight */
        pipe_state.nbegun++;
    }
    chunk_begin_finish(c);
    item *next_items = NULL;
    int next_n = 0, next_buf = 0;
    if (NULL != look_ahead && look_ahead(&next_items, &next_n, &next_buf)) {
        chunk_ahead = chunk_slot();
        chunk_begin(eng, chunk_ahead, next_items, next_n, next_buf, 0);
        pipe_state.nbegun++;
    }
    static int depth = 0;
    if (0 == depth) { const char *e = getenv("FLAPPIE_INFLIGHT"); depth = (e && atoi(e) == 3) ? NINFLIGHT - 1 : 1; }
    /* ---- a chunk of MIXED lengths goes in packed batches: what the one-read-a-row grouping below would pay for (rows x the group's longest read, group by
     * group) against what the reads hold; below 0.85 the chunk's reads are placed several to a row (ffhip_pack_plan: longest first, each into the emptiest row) in as few batches of --batch rows
     * as hold them, rows just long enough -- a batch then costs what its samples cost (nanopore-like mix: 0.07 -> 0.9+, tools/length_mix.py) */
    int packed_chunk = 0;
    if (c->m2 > 0 && pack_allowed(mdl) && !pack_failed) {
        unsigned long long real = 0, paid = 0;
        for (int i = 0; i < c->m2; ) {
            const size_t longest = c->group[i]->res.rt.end - c->group[i]->res.rt.start;
            int g = 1;
            real += longest;
            while (i + g < c->m2 && g < args.batch && 4 * (c->group[i + g]->res.rt.end - c->group[i + g]->res.rt.start) >= 3 * longest) { real += c->group[i + g]->res.rt.end - c->group[i + g]->res.rt.start; g++; }
            paid += (unsigned long long)longest * (unsigned long long)(4 * g < args.batch ? 16 * ((g + 15) / 16) : args.batch);
            i += g;
        }
        packed_chunk = (double)real < 0.85 * (double)paid;
    }
    if (packed_chunk) {
        size_t *ns = malloc(c->m2 * sizeof(size_t));
        int *slot_of = malloc(c->m2 * sizeof(int)), *off_of = malloc(c->m2 * sizeof(int)), *sl2 = malloc(c->m2 * sizeof(int)), *of2 = malloc(c->m2 * sizeof(int));
        item **sel = malloc(c->m2 * sizeof(item *)), **rest = malloc(c->m2 * sizeof(item *));
        int nleft = c->m2;
        memcpy(rest, c->group, c->m2 * sizeof(item *));
        /* The SHAPE of this chunk's batch objects is fixed by the chunk as a whole -- rows long enough for its longest read and for everything in ONE batch of --batch rows
         * (5 % slack for the gaps and the fit; at most PACK_ROW_MAX samples unless a read is longer), capacities in pack_row_cap's steps, as many rows (<= --batch) as the
         * device's memory takes at that length (ffhip_pack_rows_for: 1024 rows of 237 568 samples at 256 hidden units are 160 GB) -- and every batch of the chunk is planned
         * into it: what one batch does not hold goes into the next, whose reads are shorter (longest first) and fit the same object. */
        unsigned long long total_all = 0;
        for (int i = 0; i < nleft; i++) total_all += rest[i]->res.rt.end - rest[i]->res.rt.start;
        const size_t longest_all = rest[0]->res.rt.end - rest[0]->res.rt.start;
        size_t cap_all = (size_t)((double)total_all / (double)args.batch * 1.05) + 64 * ffhip_model_pack_gap(mdl);
        if (cap_all < longest_all + 64) cap_all = longest_all + 64;
        if (cap_all > PACK_ROW_MAX && longest_all + 64 <= PACK_ROW_MAX) cap_all = PACK_ROW_MAX;
        size_t cap_obj = pack_row_cap(cap_all);
        /* Two objects of --batch rows do not fit (H = 256: 1024 rows of 237 568 samples are 160 GB each) but ONE does: the full launch is worth more than setting a batch up
         * beside the one that runs (k_lstm_pack at 1024 rows 200+ Msamples/s, the forms for 512 rows 155; a packed batch's set-up is milliseconds) -- this chunk's batches
         * go through one object, each collected before the next is set up */
        int single = 0;
        int rows_mem = ffhip_pack_rows_for(mdl, args.batch, cap_obj, 2);
        if (rows_mem < args.batch) {
            /* (... or at least half again as many rows as two objects would have: the r941_5mC shape -- stride 2, 2.5 x the blocks a sample -- on 200 000-sample reads takes
             * 272 rows twice or 544 once; rows are what fills the chip) */
            const int rows_one = ffhip_pack_rows_for(mdl, args.batch, cap_obj, 1);
            if (rows_one >= args.batch || 2 * rows_one >= 3 * rows_mem) { single = 1; rows_mem = rows_one; }
        }
        if (rows_mem < args.batch && rows_mem >= args.batch / 2) rows_mem = args.batch / 2;      /* (half a launch's rows keep a form of the layer kernel that fills the chip; 7/8 of one does not) */
        /* ... unless a full-size object with rows long enough is there already: its shape stands (a shorter chunk could take more rows of shorter rows -- and pay seconds of
         * hipMalloc for them, chunk after chunk) */
        for (int k = 0; k < NINFLIGHT; k++)
            if (pack_cache[k].b && pack_cache[k].full && pack_cache[k].cap >= cap_obj) { cap_obj = pack_cache[k].cap; rows_mem = pack_cache[k].rows; single = pack_cache[k].single; break; }
        while (nleft > 0 && ns && slot_of && off_of && sl2 && of2 && sel && rest) {
            unsigned long long total = 0;
            for (int i = 0; i < nleft; i++) { ns[i] = rest[i]->res.rt.end - rest[i]->res.rt.start; total += ns[i]; }
            /* this batch: rows just long enough for what is left (a launch runs as long as its longest row), and no more rows than the samples left fill */
            size_t cap = (size_t)((double)total / (double)rows_mem * 1.05) + 64 * ffhip_model_pack_gap(mdl);
            if (cap < ns[0] + 64) cap = ns[0] + 64;
            cap = (cap + 1023) & ~(size_t)1023;
            if (cap > cap_obj) cap = cap_obj;
            int rows = (int)(((double)total * 1.10 / (double)cap) / 16.0 + 2.0) * 16;
            if (rows > rows_mem) rows = rows_mem;
            int placed = 0;
            for (int tries = 0; tries < 6; tries++) {
                placed = ffhip_pack_plan(mdl, rows, cap, nleft, ns, slot_of, off_of);
                if (placed == nleft) break;
                if (rows < rows_mem) { rows = (rows + 32 < rows_mem) ? rows + 32 : rows_mem; continue; }      /* the fit left reads over: more rows, ... */
                if (cap >= cap_obj) break;                                                                    /* ... or longer ones, as far as the object goes */
                cap = ((size_t)((double)cap * 1.06) + 1023) & ~(size_t)1023;
                if (cap > cap_obj) cap = cap_obj;
            }
            if (placed <= 0) {                             /* (no read is dropped for it: what is left of the chunk goes one read a row) */
                warnx("packed batch: no read fits a row of %zu samples; the chunk's %d remaining read(s) go to one-read-a-row batches", cap, nleft);
                run_groups(eng, mdl, c, rest, nleft, hdf5out, depth);
                break;
            }
            int nsel = 0, nrest = 0;
            for (int i = 0; i < nleft; i++) {
                if (slot_of[i] >= 0) { sel[nsel] = rest[i]; sl2[nsel] = slot_of[i]; of2[nsel] = off_of[i]; nsel++; }
                else rest[nrest++] = rest[i];
            }
            if (single) {                                  /* one object: nothing in flight while it is set up, and no second object alive */
                pipe_collect_all(mdl, hdf5out);
                pipe_state.slot = 0;
                for (int k = 1; k < NINFLIGHT; k++) if (pack_cache[k].b) { ffhip_batch_destroy(pack_cache[k].b); pack_cache[k].b = NULL; pack_cache[k].cap = 0; }
            }
            pending_batch cur = submit_packed(eng, mdl, c->prep, sel, nsel, sl2, of2, rows, rows_mem, cap, cap_obj, rs_chunk_cap, pipe_state.slot, single);
            if (NULL == cur.b && NULL == pack_cache[pipe_state.slot].b) {
                /* the object could not be created (device memory): no read is dropped for that -- this batch's reads and the chunk's remaining ones go one read a row,
                 * and so does the rest of the run */
                warnx("packed batches are off for the rest of this run (no memory for %d rows of %zu samples)", rows_mem, cap_obj);
                pack_failed = 1;
                free(cur.idx); free(cur.its);
                pipe_collect_all(mdl, hdf5out);                /* (nothing in flight any more: the packed objects that were made give their memory back) */
                for (int k = 0; k < NINFLIGHT; k++) if (pack_cache[k].b) { ffhip_batch_destroy(pack_cache[k].b); pack_cache[k].b = NULL; pack_cache[k].cap = 0; }
                memcpy(sel + nsel, rest, nrest * sizeof(item *));
                qsort(sel, nsel + nrest, sizeof(item *), by_length_desc);
                run_groups(eng, mdl, c, sel, nsel + nrest, hdf5out, depth);
                break;
            }
            cur.owner = c;
            c->submitted++;
            while (pipe_state.nfifo >= depth) pipe_collect_oldest(mdl, hdf5out);
            pipe_state.fifo[pipe_state.nfifo++] = cur;
            pipe_state.slot = single ? 0 : (pipe_state.slot + 1) % (depth + 1);
            nleft = nrest;
        }
        free(ns); free(slot_of); free(off_of); free(sl2); free(of2); free(sel); free(rest);
    } else run_groups(eng, mdl, c, c->group, c->m2, hdf5out, depth);
    c->all_submitted = 1;
    /* A chunk without a single batch (every read failed) collects nothing on its own account: the batch still in flight belongs
     * to an OLDER chunk, whose reader buffer is only released when it is written -- two such chunks in a row and the reader
     * thread would wait for that buffer while this thread waits for the reader.  Collect it now. */
    if (0 == c->m2) pipe_collect_all(mdl, hdf5out);
    pipe_finish_ready(hdf5out);
}

static void run_groups(struct ffhip_engine *eng, const struct ffhip_model *mdl, struct chunk_ctx *c, item **group, int m2, hid_t hdf5out, int depth) {
    for (int i = 0; i < m2; ) {
        const size_t longest = group[i]->res.rt.end - group[i]->res.rt.start;
        int g = 1;
        while (i + g < m2 && g < args.batch && 4 * (group[i + g]->res.rt.end - group[i + g]->res.rt.start) >= 3 * longest) g++;
        pending_batch cur = submit_batch(eng, mdl, c->prep, group + i, g, pipe_state.slot);
        cur.owner = c;
        c->submitted++;
        /* default: one batch runs while the next is set up.  FLAPPIE_INFLIGHT=3 keeps two on the GPU while the third is set up: no
         * measurable gain on 4000-sample reads (80-92 against 84-87 Msamples/s, run-to-run noise), and a third batch object costs
         * long reads another 10+ GB of workspace and ~1 s of start-up */
        while (pipe_state.nfifo >= depth) pipe_collect_oldest(mdl, hdf5out);           /* may complete and write an earlier chunk */
        pipe_state.fifo[pipe_state.nfifo++] = cur;
        pipe_state.slot = (pipe_state.slot + 1) % (depth + 1);       /* depth in flight + the one being set up: no more batch objects than that */
        i += g;
    }
}

/* Without the reader thread (FLAPPIE_DEBUG=no_reader_thread) this thread fills the reader buffers itself: buffer k may only be
 * overwritten once the chunk that last used it has been WRITTEN -- by the writer thread, possibly still at work. */
static void pipe_wait_slot_written(void) {
    chunk_ctx *c = &pipe_state.ctx[pipe_state.nbegun % NCHUNKBUF];
    if (writer.started != 1) return;               /* no writer thread: chunks are written by this thread, in pipe_finish_ready */
    pthread_mutex_lock(&writer.mu);
    while (__atomic_load_n(&c->live, __ATOMIC_ACQUIRE)) pthread_cond_wait(&writer.cv, &writer.mu);
    pthread_mutex_unlock(&writer.mu);
}

static void pipe_drain(const struct ffhip_model *mdl, hid_t hdf5out) {
    pipe_collect_all(mdl, hdf5out);
    pipe_finish_ready(hdf5out);
    writer_finish();
}

/* ---- input side: the list of files (flappie.c:336-358), read one chunk ahead of the GPU by a reader thread ---- */
typedef struct { char **path; size_t n, cap; } file_list;

static int by_path(const void *a, const void *b) { return strcmp(*(char *const *)a, *(char *const *)b); }

/* --shard-by-size: the shard of every file of the sorted list, balanced by bytes (a single-read fast5 file's size follows its sample
 * count): files in order of decreasing size, ties by position, each to the shard that holds the fewest bytes so far (lowest index on a
 * tie) -- flappie_amd/shard.py::partition_reads, SURVEY.md section 8e.  Every process of a sharded run computes the same table. */
typedef struct { off_t size; size_t idx; } sized_file;
static int by_size_desc(const void *a, const void *b) {
    const sized_file *x = a, *y = b;
    if (x->size != y->size) return x->size < y->size ? 1 : -1;
    return x->idx < y->idx ? -1 : (x->idx > y->idx ? 1 : 0);
}
static int *shards_by_size(char **path, size_t n, int nshard) {
    sized_file *sf = malloc((n ? n : 1) * sizeof(*sf));
    int *shard = malloc((n ? n : 1) * sizeof(int));
    unsigned long long *load = calloc((size_t)nshard, sizeof(*load));
    if (NULL == sf || NULL == shard || NULL == load) errx(EXIT_FAILURE, "out of memory");
    for (size_t f = 0; f < n; f++) {
        struct stat st;
        sf[f].size = (0 == stat(path[f], &st)) ? st.st_size : 0;
        sf[f].idx = f;
    }
    qsort(sf, n, sizeof(*sf), by_size_desc);
    for (size_t k = 0; k < n; k++) {
        int best = 0;
        for (int g = 1; g < nshard; g++) if (load[g] < load[best]) best = g;
        shard[sf[k].idx] = best;
        load[best] += (unsigned long long)sf[k].size;
    }
    free(sf); free(load);
    return shard;
}

static void list_files(file_list *fl) {
    const int reads_limit = (args.nshard >= 1) ? 0 : args.limit;      /* a shard is cut from the whole list, then limited */
    for (int fn = 0; args.files && args.files[fn]; fn++) {
        if (reads_limit > 0 && (int)fl->n >= reads_limit) break;
        glob_t globbuf;
        /* a directory means every .fast5 file inside it (flappie.c:341-353) */
        const size_t rootlen = strlen(args.files[fn]);
        char *globpath = calloc(rootlen + 9, sizeof(char));
        memcpy(globpath, args.files[fn], rootlen);
        DIR *dirp = opendir(args.files[fn]);
        if (NULL != dirp) { memcpy(globpath + rootlen, "/*.fast5", 8); closedir(dirp); }
        const int globret = glob(globpath, GLOB_NOSORT, NULL, &globbuf);
        free(globpath);
        if (0 != globret) {
            if (GLOB_NOMATCH == globret) warnx("File or directory \"%s\" does not exist or no fast5 files found.", args.files[fn]);
            globfree(&globbuf);
            continue;
        }
        for (size_t f2 = 0; f2 < globbuf.gl_pathc; f2++) {
            if (reads_limit > 0 && (int)fl->n >= reads_limit) break;
            if (fl->n == fl->cap) { fl->cap = fl->cap ? 2 * fl->cap : 1024; fl->path = realloc(fl->path, fl->cap * sizeof(char *)); }
            fl->path[fl->n++] = strdup(globbuf.gl_pathv[f2]);
        }
        globfree(&globbuf);
    }
    if (args.nshard >= 1) {
        /* every process of a sharded run must see the same order: sort, keep every n-th file starting at g */
        qsort(fl->path, fl->n, sizeof(char *), by_path);
        int *of = args.shard_by_size ? shards_by_size(fl->path, fl->n, args.nshard) : NULL;
        size_t kept = 0;
        for (size_t f = 0; f < fl->n; f++) {
            const int g = of ? of[f] : (int)(f % (size_t)args.nshard);
            if (g == args.shard && (args.limit <= 0 || (int)kept < args.limit)) fl->path[kept++] = fl->path[f];
            else free(fl->path[f]);
        }
        free(of);
        fl->n = kept;
    }
}

typedef struct {
    int chunk_cap;
    item *items[NCHUNKBUF];              /* one more than the chunks that can be unfinished at a time (one per batch in flight) */
    int nitem[NCHUNKBUF], last[NCHUNKBUF];      /* last: no read follows this chunk */
    sem_t filled[NCHUNKBUF], empty[NCHUNKBUF];
} reader_state;

/* ---- reader PROCESSES.  Opening and reading a single-read fast5 costs ~0.1-0.15 ms of CPU in libhdf5 (~6800 files/s on one
 * core; since round 6 read_raw walks the files it knows itself, host/fast5_raw.c: ~10 us, and libhdf5 is the fall-back), this libhdf5 is not thread-safe, and one MI355X consumes 15-20 000 reads of 4000 samples per second: one reader
 * thread caps the binary at less than half of what the kernels deliver.  So the files are read by `--readers` child
 * processes, forked BEFORE the HIP runtime starts (a fork of a process with a live GPU context is not supported): child k
 * reads files k, k + R, k + 2R ... in order (read_raw, fast5_interface.c:231-318, with the pA scaling of flappie.c:248) and
 * streams {nsample, uuid, samples} records down its own pipe; the parent's reader thread takes file f from pipe f % R, so
 * the input order is kept.  Children run ahead by what a pipe holds (1 MiB: ~50 reads each). */
typedef struct { pid_t pid; int fd; int dead; } reader_proc;
static reader_proc *rprocs = NULL;
static int nrproc = 0;

static int write_all(int fd, const void *buf, size_t n) {
    const char *p = buf;
    while (n > 0) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) { if (EINTR == errno) continue; return -1; }
        p += w; n -= (size_t)w;
    }
    return 0;
}
static int read_all(int fd, void *buf, size_t n) {
    char *p = buf;
    while (n > 0) {
        const ssize_t r = read(fd, p, n);
        if (r < 0) { if (EINTR == errno) continue; return -1; }
        if (0 == r) return -1;
        p += r; n -= (size_t)r;
    }
    return 0;
}

/* A record of a reader's pipe: this header, the uuid, the samples.  REC_FLOAT: a single-read file, its samples as picoampere floats (one record a file, as ever);
 * REC_DAC: a read of a multi-read file, int16 DAC values as the file holds them and the calibration in the header (half the bytes down the pipe, into pinned memory
 * and up to the device); REC_SKIP: a read of a multi-read file that could not be read (the child said why); REC_EOF: behind the last read of a multi-read file. */
enum { REC_FLOAT = 0, REC_DAC = 1, REC_EOF = 2, REC_SKIP = 3 };
typedef struct { uint64_t nsample, uuid_len; uint32_t kind; float offset, raw_unit; uint32_t pad; } rec_hdr;

static void reader_child(const file_list *fl, int k, int R, int fd) {
    signal(SIGPIPE, SIG_IGN);            /* a parent that went away is a failed write, not a signal (the PARENT keeps the default: `flappie ... | head` ends) */
    long kill_k = -1, kill_f = -1, kill_r = 0;      /* tests: FLAPPIE_DEBUG=kill_reader=k:f[:r] -- child k dies (SIGKILL) when it reaches file index f (read r of it, a multi-read file) */
    const char *kill_env = cli_dbg("kill_reader");
    if (kill_env && sscanf(kill_env, "%ld:%ld:%ld", &kill_k, &kill_f, &kill_r) < 2) kill_k = -1;
    for (size_t f = (size_t)k; f < fl->n; f += (size_t)R) {
        if (kill_k == k && (long)f >= kill_f && (0 == kill_r || (long)f > kill_f)) raise(SIGKILL);
        fast5_multi *multi = NULL;
        raw_table rt = read_raw_or_multi(fl->path[f], true, &multi);
        if (NULL != multi) {
            fast5_dac_read dr;
            int rc;
            for (long r = 0; 0 != (rc = fast5_multi_next(multi, &dr)); r++) {
                if (kill_k == k && (long)f == kill_f && r >= kill_r) raise(SIGKILL);
                rec_hdr h = { rc > 0 ? (uint64_t)dr.n : 0, (rc > 0 && NULL != dr.uuid) ? (uint64_t)strlen(dr.uuid) : 0, rc > 0 ? REC_DAC : REC_SKIP, dr.offset, dr.raw_unit, 0 };
                if (0 != write_all(fd, &h, sizeof(h)) || (h.uuid_len && 0 != write_all(fd, dr.uuid, h.uuid_len)) ||
                    (h.nsample && 0 != write_all(fd, dr.dac, h.nsample * sizeof(int16_t)))) _exit(1);
                free(dr.dac);
                free(dr.uuid);
            }
            fast5_multi_close(multi);
            rec_hdr h = { 0, 0, REC_EOF, 0.0f, 0.0f, 0 };
            if (0 != write_all(fd, &h, sizeof(h))) _exit(1);
            continue;
        }
        rec_hdr h = { (NULL != rt.raw) ? (uint64_t)rt.n : 0, (NULL != rt.uuid && NULL != rt.raw) ? (uint64_t)strlen(rt.uuid) : 0, REC_FLOAT, 0.0f, 0.0f, 0 };
        if (0 != write_all(fd, &h, sizeof(h)) || (h.uuid_len && 0 != write_all(fd, rt.uuid, h.uuid_len)) ||
            (h.nsample && 0 != write_all(fd, rt.raw, h.nsample * sizeof(float)))) _exit(1);      /* the parent went away */
        free(rt.raw);
        free(rt.uuid);
    }
    _exit(0);
}

static void start_reader_procs(const file_list *fl, int R) {
    if (R <= 0 || 0 == fl->n) return;
    if ((size_t)R > fl->n) R = (int)fl->n;
    rprocs = calloc((size_t)R, sizeof(reader_proc));
    fflush(NULL);
    for (int k = 0; k < R; k++) {
        int pfd[2];
        if (0 != pipe(pfd)) errx(EXIT_FAILURE, "could not create a pipe for reader %d", k);
        const pid_t pid = fork();
        if (pid < 0) errx(EXIT_FAILURE, "could not fork reader %d", k);
        if (0 == pid) {
            close(pfd[0]);
            for (int j = 0; j < k; j++) close(rprocs[j].fd);
            reader_child(fl, k, R, pfd[1]);
        }
        close(pfd[1]);
#ifdef F_SETPIPE_SZ
        (void)fcntl(pfd[0], F_SETPIPE_SZ, 1 << 20);
#endif
        rprocs[k].pid = pid;
        rprocs[k].fd = pfd[0];
        nrproc = k + 1;
    }
}

/* ---- the stream of reads: file after file, a multi-read file read after read (in increasing strcmp order of its group names: the cursor's order).
 * next_item fills one item per read; a file -- or a read of a multi-read file -- that could not be read is an item without a signal ("No basecall returned").
 *
 * A reader child that dies (libhdf5 crashing on a corrupt file, an OOM kill) takes its stripe with it: the file it died on is reported unreadable -- of a
 * multi-read file the reads not yet delivered are lost --, every LATER file of the stripe is read in this process instead (as with --readers 0), and the exit
 * status of the run says that a reader failed.  A stream cut in the middle of a record is out of sync and handled the same way. */
static struct {
    const file_list *fl;
    size_t f;                    /* the file the next read comes from */
    fast5_multi *cur;            /* in-process: the cursor over file f */
    int in_multi;                /* from a reader process: file f is a multi-read file and its end-of-file record has not come yet */
    long nitems;                 /* --limit counts reads */
    item held; int have_held;    /* read_chunk looked one read ahead */
} in;

static void reader_lost(size_t f, const char *path) {
    reader_proc *rp = &rprocs[f % (size_t)nrproc];
    rp->dead = 1;
    reader_failures++;
    warnx("reader process %zu ended early at %s; the rest of its files are read in-process", f % (size_t)nrproc, path);
}

static void item_init(item *it, const char *path) {
    memset(it, 0, sizeof(*it));
    it->filename = strdup(path);
    it->rm_ref = -1;
    it->tr_ref = -1;
}
static void item_from_dac(item *it, const char *path, const fast5_dac_read *dr) {
    item_init(it, path);
    it->from_multi = 1;
    if (NULL == dr) return;
    it->res.rt = (raw_table){ dr->uuid, dr->n, 0, dr->n, NULL };
    it->dac = dr->dac; it->dac_offset = dr->offset; it->dac_unit = dr->raw_unit;
}

/* no call of next_item can give another read (known without reading anything) */
static int input_exhausted(void) {
    if (args.limit > 0 && in.nitems >= args.limit) return 1;
    return NULL == in.cur && !in.in_multi && in.f >= in.fl->n;
}

/* 1: *it is the next read; 0: the input has ended (or --limit reads were given out) */
static int next_item(item *it) {
    for (;;) {
        if (args.limit > 0 && in.nitems >= args.limit) return 0;
        if (NULL != in.cur) {                                               /* in-process, inside a multi-read file */
            fast5_dac_read dr;
            pthread_mutex_lock(&hdf5_lock);
            const int rc = fast5_multi_next(in.cur, &dr);
            if (0 == rc) { fast5_multi_close(in.cur); in.cur = NULL; }
            pthread_mutex_unlock(&hdf5_lock);
            if (0 == rc) { in.f++; continue; }
            item_from_dac(it, in.fl->path[in.f], rc > 0 ? &dr : NULL);
            in.nitems++;
            return 1;
        }
        if (in.f >= in.fl->n) return 0;
        const char *path = in.fl->path[in.f];
        if (nrproc > 0 && !rprocs[in.f % (size_t)nrproc].dead) {
            const int fd = rprocs[in.f % (size_t)nrproc].fd;
            rec_hdr h;
            char *uuid = NULL;
            void *samples = NULL;
            int lost = 0 != read_all(fd, &h, sizeof(h)) || h.kind > REC_SKIP || h.uuid_len > (1u << 16) || h.nsample > ((uint64_t)1 << 36);
            if (!lost && h.uuid_len) { uuid = calloc(h.uuid_len + 1, 1); lost = NULL == uuid || 0 != read_all(fd, uuid, h.uuid_len); }
            if (!lost && h.nsample) {
                const size_t bytes = h.nsample * (REC_DAC == h.kind ? sizeof(int16_t) : sizeof(float));
                samples = malloc(bytes);
                lost = NULL == samples || 0 != read_all(fd, samples, bytes);
            }
            if (lost) {
                free(uuid); free(samples);
                reader_lost(in.f, path);
                const int was_inside = in.in_multi;
                in.in_multi = 0;
                in.f++;
                if (was_inside) continue;                                   /* the reads delivered so far stand; the file's others are lost */
                item_init(it, path);                                        /* this file: whatever killed the child stays unread */
                in.nitems++;
                return 1;
            }
            if (REC_EOF == h.kind) { free(uuid); free(samples); in.in_multi = 0; in.f++; continue; }
            if (REC_FLOAT == h.kind) {
                item_init(it, path);
                if (h.nsample) it->res.rt = (raw_table){ uuid, h.nsample, 0, h.nsample, samples };
                else free(uuid);                                            /* the child could not read the file (it said why) */
                in.f++;
            } else {
                in.in_multi = 1;
                fast5_dac_read dr = { uuid, samples, h.nsample, h.offset, h.raw_unit };
                item_from_dac(it, path, (REC_DAC == h.kind && h.nsample) ? &dr : NULL);
                if (NULL == it->dac) { free(uuid); free(samples); }
            }
            in.nitems++;
            return 1;
        }
        /* in-process: --readers 0, or the stripe of a reader that died */
        pthread_mutex_lock(&hdf5_lock);
        fast5_multi *multi = NULL;
        const raw_table rt = read_raw_or_multi(path, true, &multi);         /* flappie.c:248 */
        pthread_mutex_unlock(&hdf5_lock);
        if (NULL != multi) { in.cur = multi; continue; }
        item_init(it, path);
        it->res.rt = rt;
        in.f++;
        in.nitems++;
        return 1;
    }
}

static void stop_reader_procs(void) {
    for (int k = 0; k < nrproc; k++) {
        close(rprocs[k].fd);
        int st = 0;
        if (waitpid(rprocs[k].pid, &st, 0) == rprocs[k].pid && !rprocs[k].dead) {
            /* exit status 1 = its pipe closed under it (this process stopped reading early: --limit, an error) -- not a failure of the child */
            if (WIFSIGNALED(st)) { warnx("reader process %d was killed by signal %d", k, WTERMSIG(st)); reader_failures++; }
            else if (WIFEXITED(st) && WEXITSTATUS(st) > 1) { warnx("reader process %d exited with status %d", k, WEXITSTATUS(st)); reader_failures++; }
        }
    }
    free(rprocs);
    rprocs = NULL;
    nrproc = 0;
}

/* Mixed lengths (packed batches): a read of L samples is L / stride dependent steps of every layer, whatever else the GPU holds meanwhile -- a chunk whose longest read
 * is L should hold about --batch rows of L samples of work, or its one batch runs as long as that read with most rows empty (tools/length_mix.py: 8192 files of a
 * log-normal mix, 33 M-sample chunks: 105 of 512 rows in use).  The chunk's sample budget therefore grows with the longest read seen while it fills, up to
 * PACK_WINDOW_MAX samples and PACK_WINDOW_READS x the usual read count (the reader's buffers are that large).  Uniform reads never get there. */
#define PACK_WINDOW_MAX ((size_t)224 << 20)
#define PACK_WINDOW_READS 4
static int g_pack_window = 0;                /* set once the model is known: pack_allowed() */
static void read_chunk(int chunk_cap, item *items, int *nitem, int *last) {
    /* a chunk is up to chunk_cap reads (CHUNK_BATCHES batches of the usual 4-8 k-sample reads) -- or, with long reads, what holds about as
     * many SAMPLES but at least one batch: records leave when their chunk is done, and a 1024-read chunk of 100 000-sample reads
     * would be four seconds of GPU work with nothing written (and nothing for the writer thread to overlap).
     * A chunk holds ONE kind of read -- DAC values (multi-read files) or floats (single-read files): its preparation is one call of one entry, so the chunk is
     * cut where the kind changes (the read that changes it is held for the next chunk; nothing is converted on the host to avoid the cut). */
    size_t sample_budget = (size_t)chunk_cap * 8192, longest = 0;
    size_t nsamp = 0;
    int n = 0, read_cap = chunk_cap, kind = -1;
    const double tr0 = now_s();
    for (; n < read_cap && !(n >= args.batch && nsamp >= sample_budget); n++) {
        item *it = &items[n];
        if (in.have_held) { *it = in.held; in.have_held = 0; }
        else if (!next_item(it)) break;
        if (item_has_signal(it)) {
            const int k = NULL != it->dac;
            if (kind >= 0 && k != kind) { in.held = *it; in.have_held = 1; break; }
            kind = k;
            nsamp += it->res.rt.n;
        }
        if (g_pack_window && item_has_signal(it) && it->res.rt.n > longest) {
            longest = it->res.rt.n;
            /* (... and a twentieth more: these are RAW samples, the rows hold trimmed ones, and rows that average a little MORE than the longest read let the planner --
             * every read into the emptiest row -- end with all rows alike; at exactly --batch x longest the trimming left the rows 2.7 % under a row that holds the
             * longest read alone, and that row is what the launch lasts: fill 0.973 -> 0.99, tools/dev/pack_log.sh) */
            size_t want = (size_t)args.batch * longest + (size_t)args.batch * longest / 20;
            if (want > PACK_WINDOW_MAX) want = PACK_WINDOW_MAX;
            if (want > sample_budget) { sample_budget = want; read_cap = PACK_WINDOW_READS * chunk_cap; }
        }
    }
    t_phase[0] += now_s() - tr0;
    /* No read is taken ahead to learn whether a chunk follows (the first, small chunk goes to the GPU as soon as it is full): the input says when it is exhausted.
     * Behind the last read of a multi-read file it cannot know yet -- the cursor, or the reader's end-of-file record, says so at the next call -- so a chunk that
     * such a file's last read fills exactly is followed by an empty last one, which the main loop passes over. */
    *last = 0 == n || (!in.have_held && input_exhausted());      /* (no read at all: next_item said that the input has ended) */
    *nitem = n;
}

static void release_buffer(int buf, void *arg) { sem_post(&((reader_state *)arg)->empty[buf]); }

static void *reader_main(void *arg) {
    reader_state *rs = arg;
    int first = 1, last = 0;
    for (int k = 0; !last; k = (k + 1) % NCHUNKBUF) {
        sem_wait(&rs->empty[k]);
        /* the first chunk is one batch only, so that the GPU starts after --batch reads instead of CHUNK_BATCHES times as many */
        read_chunk(first ? rs->chunk_cap / CHUNK_BATCHES : rs->chunk_cap, rs->items[k], &rs->nitem[k], &rs->last[k]);
        first = 0;
        last = rs->last[k];
        sem_post(&rs->filled[k]);
    }
    return NULL;
}

/* pipe_chunk's look-ahead over the reader thread's buffers: buffer kn holds the next chunk if its `filled` can be taken now (the main loop then skips its own wait for it) */
static struct { reader_state *rs; int on, kn, more, taken; } la;
static int look_ahead_reader(item **items, int *n, int *buf) {
    if (!la.on || !la.more || la.taken) return 0;
    if (0 != sem_trywait(&la.rs->filled[la.kn])) {
        if (cli_dbg("pack_log")) fprintf(stderr, "look-ahead at %.3f s: the reader has not filled buffer %d yet\n", now_s() - t_program_start, la.kn);
        return 0;
    }
    la.taken = 1;
    if (0 == la.rs->nitem[la.kn]) return 0;      /* (the empty last chunk behind a multi-read file whose last read filled a chunk: nothing to prepare) */
    if (cli_dbg("pack_log")) fprintf(stderr, "look-ahead at %.3f s: buffer %d is there (%d reads)\n", now_s() - t_program_start, la.kn, la.rs->nitem[la.kn]);
    unsigned long long raw = 0;
    for (int i = 0; i < la.rs->nitem[la.kn]; i++) if (item_has_signal(&la.rs->items[la.kn][i])) raw += la.rs->items[la.kn][i].res.rt.n;
    unsigned long long least = 48ull << 20;      /* the usual chunks: their device pass is a millisecond beside the batch in flight as it is */
    const char *lm = cli_dbg("prep_ahead_min");  /* tests: FLAPPIE_DEBUG=prep_ahead_min=0 takes this path with chunks of any size */
    if (NULL != lm) least = strtoull(lm, NULL, 10);
    if (raw < least) return 0;
    *items = la.rs->items[la.kn]; *n = la.rs->nitem[la.kn]; *buf = la.kn;
    return 1;
}

/* FLAPPIE_DEBUG=segv_trace: the call stack of a crash on stderr (addresses for addr2line; development) */
static void segv_trace(int sig) {
    void *frames[48];
    const int n = backtrace(frames, 48);
    static const char msg[] = "flappie: fatal signal, call stack:\n";
    if (write(2, msg, sizeof(msg) - 1) < 0) _exit(128 + sig);
    backtrace_symbols_fd(frames, n, 2);
    _exit(128 + sig);
}

int main(int argc, char *argv[]) {
    t_program_start = now_s();
    argp_parse(&argp, argc, argv, 0, 0, NULL);
#ifdef BUILD_RUNNIE
    if ((args.rlc || args.run_scale_set) && !args.fasta) errx(EXIT_FAILURE, "--rlc and --run-scale go with --fasta");
    if (args.barcodes) errx(EXIT_FAILURE, "--barcodes is flappie's: the run-length model's records carry no base strings to search");
    if (ad_path || ad_opts) errx(EXIT_FAILURE, "--adapters is flappie's: the run-length model's records carry no base strings to search");
    if (map_path || map_opts) errx(EXIT_FAILURE, "--map is flappie's: the run-length model's records carry no base strings to place");
    if (pt_on || pt_opts) errx(EXIT_FAILURE, "--poly-tail is flappie's: the run-length model's path is not one of bases");
    if (args.remap) errx(EXIT_FAILURE, "--remap is flappie's: the run-length model's scores are not transitions between the bases of a sequence");
    if (args.truth) errx(EXIT_FAILURE, "--truth is flappie's: the run-length model's call is a list of runs");
    if (tfm_on || tfm_sam_path) errx(EXIT_FAILURE, "--truth-from-map and --map-sam are flappie's: the run-length model's call is a list of runs");
    if (rfm_on) errx(EXIT_FAILURE, "--remap-from-map is flappie's: the run-length model's scores are not transitions between the bases of a sequence");
    if (pu_path || pu_min_identity >= 0) errx(EXIT_FAILURE, "--map-pileup and --map-pileup-min-identity are flappie's: the run-length model's call is a list of runs");
    if (mm_path || mm_hi >= 0 || mm_lo >= 0 || mm_min_identity >= 0 || mm_motif || mm_combine || mm_hist_path)
        errx(EXIT_FAILURE, "--map-mods and its --map-mods-* options are flappie's: the run-length model's call is a list of runs and it has no modified base");
    if (cs_path || cs_changes_path || cs_min_depth >= 0 || cs_min_identity >= 0)
        errx(EXIT_FAILURE, "--map-consensus and its --map-consensus-* options are flappie's: the run-length model's call is a list of runs");
    if (ep_path || ep_min_identity >= 0) errx(EXIT_FAILURE, "--truth-errors and --truth-errors-min-identity are flappie's: the run-length model's call is a list of runs");
    if (args.remap_events) errx(EXIT_FAILURE, "--remap-events is flappie's: it goes with --remap, which the run-length model does not have");
    if (mods_path) errx(EXIT_FAILURE, "--remap-mods is flappie's: it goes with --remap, which the run-length model does not have");
    if (vars_path || vars_out_path || vars_opts) errx(EXIT_FAILURE, "--remap-variants is flappie's: it goes with --remap, which the run-length model does not have");
#else
    /* --barcodes: every refusal before any file or the GPU is touched */
    if (args.bc_opts && NULL == args.barcodes) errx(EXIT_FAILURE, "--barcode-window, --barcode-max-dist, --barcode-min-sep, --barcode-both-ends and --trim-barcodes go with --barcodes");
    if (args.bc_trim && (args.emit_moves || args.modbase_tags || NULL != args.trace))
        errx(EXIT_FAILURE, "--trim-barcodes does not go with --emit-moves, --modbase-tags or --trace: their positions and probabilities are the untrimmed call's");
    if (args.barcodes) {
        char why[256];
        bc_kit = flappie_barcode_kit_read(args.barcodes, why, sizeof why);
        if (NULL == bc_kit) errx(EXIT_FAILURE, "--barcodes %s: %s", args.barcodes, why);
    }
    /* --poly-tail: the options' values and what it does not go with */
    if (pt_opts && !pt_on) errx(EXIT_FAILURE, "--poly-tail-base, --poly-tail-end, --poly-tail-window, --poly-tail-min-calls, --poly-tail-max-sd, --poly-tail-gap, --poly-tail-min-windows, --poly-tail-search and --poly-tail-min-bases go with --poly-tail");
    if (pt_err[0]) errx(EXIT_FAILURE, "%s", pt_err);
    if (pt_on) {
        char why[256];
        if (0 != flappie_polytail_params(&pt_o, 1, &pt_params, why, sizeof why)) errx(EXIT_FAILURE, "%s", why);
        if (ad_split) errx(EXIT_FAILURE, "--poly-tail does not go with --split-reads: the pieces of a split read have no tail of their own");
    }
    /* --adapters: likewise */
    if (ad_opts && NULL == ad_path) errx(EXIT_FAILURE, "--adapter-max-dist, --trim-adapters, --adapter-window, --split-reads and --split-min-length go with --adapters");
    if (ad_window_set && !ad_trim && !ad_split) errx(EXIT_FAILURE, "--adapter-window goes with --trim-adapters or --split-reads");
    if (ad_min_length_set && !ad_split) errx(EXIT_FAILURE, "--split-min-length goes with --split-reads");
    if (ad_trim && (args.emit_moves || args.modbase_tags || NULL != args.trace))
        errx(EXIT_FAILURE, "--trim-adapters does not go with --emit-moves, --modbase-tags or --trace: their positions and probabilities are the untrimmed call's");
    if (ad_split && (args.emit_moves || args.modbase_tags || NULL != args.trace || NULL != args.remap || NULL != args.truth))
        errx(EXIT_FAILURE, "--split-reads does not go with --emit-moves, --modbase-tags, --trace, --remap or --truth: they describe the read as one molecule");
    if (ad_path) {
        char why[256];
        ad_kit = flappie_adapter_kit_read(ad_path, why, sizeof why);
        if (NULL == ad_kit) errx(EXIT_FAILURE, "--adapters %s: %s", ad_path, why);
    }
    /* --map: likewise */
    if (map_opts && NULL == map_path) errx(EXIT_FAILURE, "--map-out, --map-window, --map-max-error and --map-records go with --map");
    if (map_path && NULL == map_out_path) errx(EXIT_FAILURE, "--map and --map-out go together");
    /* ... and --truth-from-map, which stands on it */
    if (tfm_on && NULL == map_path) errx(EXIT_FAILURE, "--truth-from-map goes with --map: it aligns a call to the stretch --map placed it on");
    if (tfm_on && NULL != args.truth) errx(EXIT_FAILURE, "--truth-from-map does not go with --truth: a call is aligned to one truth, the file's record or the mapped stretch");
    if (tfm_on && NULL == args.truth_out) errx(EXIT_FAILURE, "--truth-from-map and --truth-out go together");
    if (tfm_sam_path && !tfm_on) errx(EXIT_FAILURE, "--map-sam goes with --truth-from-map");
    /* --remap-from-map, which stands on --map too: the sequences are the mapped stretches, which only the device has when the run is made */
    if (rfm_on && NULL == map_path) errx(EXIT_FAILURE, "--remap-from-map goes with --map: it maps a read's signal to the stretch --map placed its call on");
    if (rfm_on && NULL != args.remap) errx(EXIT_FAILURE, "--remap-from-map does not go with --remap: a read's signal is mapped to one sequence, the file's record or the mapped stretch");
    if (rfm_on && mods_path) errx(EXIT_FAILURE, "--remap-from-map does not go with --remap-mods: the sites are listed from sequences the host has before the run, and the mapped stretches are not known then");
    if (rfm_on && (vars_path || vars_out_path || vars_opts))
        errx(EXIT_FAILURE, "--remap-from-map does not go with --remap-variants: variants are given in the coordinates of a sequence the host has before the run, and the mapped stretches are not known then");
    if (rfm_on && NULL == args.remap_out) errx(EXIT_FAILURE, "--remap-from-map and --remap-out go together");
    if (rfm_on && ad_split) errx(EXIT_FAILURE, "--split-reads does not go with --remap-from-map: it describes the read as one molecule");
    if (pu_path && !tfm_on) errx(EXIT_FAILURE, "--map-pileup goes with --truth-from-map: it counts what the alignments say");
    if (pu_min_identity >= 0 && NULL == pu_path) errx(EXIT_FAILURE, "--map-pileup-min-identity goes with --map-pileup");
    /* --map-mods: likewise; the thresholds' defaults read p >= 0.8 and p < 0.2 of ml = floor(256 p) */
    if ((mm_hi >= 0 || mm_lo >= 0 || mm_min_identity >= 0 || mm_motif || mm_combine || mm_hist_path) && NULL == mm_path)
        errx(EXIT_FAILURE, "--map-mods-hi, --map-mods-lo, --map-mods-min-identity, --map-mods-motif, --map-mods-combine-strands and --map-mods-hist go with --map-mods");
    if (mm_path && !tfm_on) errx(EXIT_FAILURE, "--map-mods goes with --truth-from-map: it counts what the alignments say");
    if (mm_path && !flappie_model_has_modbase(args.model))      /* (the registry knows: before any file or the GPU is touched) */
        errx(EXIT_FAILURE, "--map-mods needs a model with a modified base (r941_5mC); \"%s\" has none", flappie_model_string(args.model));
    if (mm_path) {
        if (mm_hi < 0) mm_hi = 205;
        if (mm_lo < 0) mm_lo = 50;
        if (mm_lo >= mm_hi) errx(EXIT_FAILURE, "--map-mods-lo (%d) must be below --map-mods-hi (%d)", mm_lo, mm_hi);
        if (mm_combine && mm_motif && 0 != strcmp(mm_motif, "CG")) errx(EXIT_FAILURE, "--map-mods-combine-strands goes with the motif CG: a lone C has no partner on the other strand");
    }
    /* --map-consensus: likewise; a depth of 3 is the least at which two agreeing calls outvote a third */
    if ((cs_changes_path || cs_min_depth >= 0 || cs_min_identity >= 0) && NULL == cs_path)
        errx(EXIT_FAILURE, "--map-consensus-changes, --map-consensus-min-depth and --map-consensus-min-identity go with --map-consensus");
    if (cs_path && !tfm_on) errx(EXIT_FAILURE, "--map-consensus goes with --truth-from-map: it counts what the alignments say");
    if (cs_path && cs_min_depth < 0) cs_min_depth = 3;
    /* --truth-errors: the alignments of either truth mode, classed */
    if (ep_min_identity >= 0 && NULL == ep_path) errx(EXIT_FAILURE, "--truth-errors-min-identity goes with --truth-errors");
    if (ep_path && !tfm_on && NULL == args.truth) errx(EXIT_FAILURE, "--truth-errors goes with --truth or --truth-from-map: it counts what the alignments say");
    if (map_path) {
        char why[256];
        mp_ref = flappie_map_ref_read(map_path, why, sizeof why);
        if (NULL == mp_ref) errx(EXIT_FAILURE, "--map %s: %s", map_path, why);
        if (NULL == (mp_out = fopen(map_out_path, "w"))) errx(EXIT_FAILURE, "--map-out %s: cannot be written", map_out_path);
        if (map_recs_path && NULL == (mp_recs = fopen(map_recs_path, "w"))) errx(EXIT_FAILURE, "--map-records %s: cannot be written", map_recs_path);
    }
    /* --remap: likewise */
    if (!rfm_on && (NULL == args.remap) != (NULL == args.remap_out)) errx(EXIT_FAILURE, "--remap and --remap-out go together");
    if (args.remap_band_set && NULL == args.remap && !rfm_on) errx(EXIT_FAILURE, "--remap-band goes with --remap");
    if (args.remap_events && NULL == args.remap && !rfm_on) errx(EXIT_FAILURE, "--remap-events goes with --remap");
    if (mods_path && NULL == args.remap) errx(EXIT_FAILURE, "--remap-mods goes with --remap");
    if ((mods_context_set || mods_all_paths) && NULL == mods_path) errx(EXIT_FAILURE, "--remap-mods-context and --remap-mods-all-paths go with --remap-mods");
    if (mods_path && !flappie_model_has_modbase(args.model))      /* (the registry knows: before any file or the GPU is touched) */
        errx(EXIT_FAILURE, "--remap-mods needs a model with a modified base (r941_5mC); \"%s\" has none", flappie_model_string(args.model));
    if (vars_path && NULL == args.remap) errx(EXIT_FAILURE, "--remap-variants goes with --remap");
    if ((vars_opts || vars_out_path) && NULL == vars_path) errx(EXIT_FAILURE, "--remap-variants-out, --remap-variants-context and --remap-variants-all-paths go with --remap-variants");
    if (vars_path && NULL == vars_out_path) errx(EXIT_FAILURE, "--remap-variants and --remap-variants-out go together");
    if (args.remap) {
        char why[256];
        rm_refs = flappie_remap_refs_read(args.remap, flappie_model_has_modbase(args.model) ? "ACGTZ" : "ACGT", why, sizeof why);
        if (NULL == rm_refs) errx(EXIT_FAILURE, "--remap %s: %s", args.remap, why);
        for (int k = 0; k < rm_refs->n; k++)
            if (rm_refs->bad[k]) warnx("--remap: record %s holds a letter outside the model's alphabet: its read is not mapped (status 2)", rm_refs->name[k]);
        if (NULL == (rm_out = fopen(args.remap_out, "w"))) errx(EXIT_FAILURE, "--remap-out %s: cannot be written", args.remap_out);
        if (args.remap_events && NULL == (ev_out = fopen(args.remap_events, "w"))) errx(EXIT_FAILURE, "--remap-events %s: cannot be written", args.remap_events);
        if (mods_path && NULL == (md_out = fopen(mods_path, "w"))) errx(EXIT_FAILURE, "--remap-mods %s: cannot be written", mods_path);
        if (vars_path) {
            vr_vars = flappie_variants_read(vars_path, rm_refs, flappie_model_has_modbase(args.model) ? "ACGTZ" : "ACGT", why, sizeof why);
            if (NULL == vr_vars) errx(EXIT_FAILURE, "--remap-variants %s: %s", vars_path, why);
            for (int k = 0; k < FLAPPIE_VARIANTS_KINDS; k++)
                if (vr_vars->skipped[k]) warnx("--remap-variants: line %zu %s: it is skipped, and %llu like it (%s)", vr_vars->skipped_line[k], flappie_variants_kind(k),
                                               vr_vars->skipped[k] - 1, vr_vars->skipped_text[k]);
            if (NULL == (vr_done = calloc(rm_refs->n > 0 ? rm_refs->n : 1, 1))) errx(EXIT_FAILURE, "--remap-variants %s: out of memory", vars_path);
            if (NULL == (vr_out = fopen(vars_out_path, "w"))) errx(EXIT_FAILURE, "--remap-variants-out %s: cannot be written", vars_out_path);
        }
    }
    if (rfm_on) {
        if (NULL == (rm_out = fopen(args.remap_out, "w"))) errx(EXIT_FAILURE, "--remap-out %s: cannot be written", args.remap_out);
        if (args.remap_events && NULL == (ev_out = fopen(args.remap_events, "w"))) errx(EXIT_FAILURE, "--remap-events %s: cannot be written", args.remap_events);
    }
    /* --truth: likewise */
    if (!tfm_on && (NULL == args.truth) != (NULL == args.truth_out)) errx(EXIT_FAILURE, "--truth and --truth-out go together");
    if (args.truth_band_set && NULL == args.truth && !tfm_on) errx(EXIT_FAILURE, "--truth-band goes with --truth or --truth-from-map");
    if (tfm_on) {
        if (NULL == (tr_out = fopen(args.truth_out, "w"))) errx(EXIT_FAILURE, "--truth-out %s: cannot be written", args.truth_out);
        if (tfm_sam_path) {
            if (NULL == (tfm_sam = fopen(tfm_sam_path, "w"))) errx(EXIT_FAILURE, "--map-sam %s: cannot be written", tfm_sam_path);
            flappie_align_write_sam_header(tfm_sam, mp_ref);
        }
        if (pu_path && NULL == (pu_out = fopen(pu_path, "w"))) errx(EXIT_FAILURE, "--map-pileup %s: cannot be written", pu_path);
        if (mm_path && NULL == (mm_out = fopen(mm_path, "w"))) errx(EXIT_FAILURE, "--map-mods %s: cannot be written", mm_path);
        if (mm_hist_path && NULL == (mm_hist = fopen(mm_hist_path, "w"))) errx(EXIT_FAILURE, "--map-mods-hist %s: cannot be written", mm_hist_path);
        if (cs_path && NULL == (cs_out = fopen(cs_path, "w"))) errx(EXIT_FAILURE, "--map-consensus %s: cannot be written", cs_path);
        if (cs_changes_path && NULL == (cs_changes = fopen(cs_changes_path, "w"))) errx(EXIT_FAILURE, "--map-consensus-changes %s: cannot be written", cs_changes_path);
    }
    if (args.truth) {
        char why[256];
        tr_refs = flappie_remap_refs_read(args.truth, flappie_model_has_modbase(args.model) ? "ACGTZ" : "ACGT", why, sizeof why);
        if (NULL == tr_refs) errx(EXIT_FAILURE, "--truth %s: %s", args.truth, why);
        for (int k = 0; k < tr_refs->n; k++)
            if (tr_refs->bad[k]) warnx("--truth: record %s holds a letter outside the model's alphabet: its read is not aligned (status 2)", tr_refs->name[k]);
        if (NULL == (tr_out = fopen(args.truth_out, "w"))) errx(EXIT_FAILURE, "--truth-out %s: cannot be written", args.truth_out);
    }
    if (ep_path && NULL == (ep_out = fopen(ep_path, "w"))) errx(EXIT_FAILURE, "--truth-errors %s: cannot be written", ep_path);
    if (args.modbase_tags && !flappie_model_has_modbase(args.model))      /* (the registry knows: before any file or the GPU is touched) */
        errx(EXIT_FAILURE, "--modbase-tags needs a model with a modified base (r941_5mC); \"%s\" has none", flappie_model_string(args.model));
#endif
    if (cli_dbg("segv_trace")) { signal(SIGSEGV, segv_trace); signal(SIGABRT, segv_trace); signal(SIGBUS, segv_trace); }
    if (NULL == args.output) args.output = stdout;
    const double t_start = now_s();
    file_list fl = { NULL, 0, 0 };
    list_files(&fl);
    const double t_listed = now_s();
    if (!cli_dbg("no_numa_bind")) { const char *dev = getenv("FLAPPIE_HIP_DEVICE"); (void)bind_to_gpu_numa(dev ? atoi(dev) : 0); }
    if (cli_dbg("list_only")) {             /* the files this process would call, one per line -- no GPU touched (tests, tools/host_scaling.py) */
        for (size_t f = 0; f < fl.n; f++) printf("%s\n", fl.path[f]);
        return EXIT_SUCCESS;
    }
    start_reader_procs(&fl, cli_dbg("no_reader_thread") ? 0 : args.readers);      /* before the HIP runtime and libhdf5 are touched here */
    const struct ffhip_model *mdl = flappie_hip_model(args.model);
    if (NULL == mdl) { stop_reader_procs(); errx(EXIT_FAILURE, "model \"%s\" is not available (set FLAPPIE_MODEL_DIR)", flappie_model_string(args.model)); }
#ifndef BUILD_RUNNIE
    if (args.emit_moves && ffhip_model_stride(mdl) > 127) {      /* (mv:B:c carries the stride as an int8; no model of the registry has such a stride) */
        stop_reader_procs();
        errx(EXIT_FAILURE, "--emit-moves: the stride of model \"%s\" (%zu samples a block) does not fit the mv tag's int8", flappie_model_string(args.model), ffhip_model_stride(mdl));
    }
#endif
    struct ffhip_engine *eng = flappie_hip_engine();
#ifndef BUILD_RUNNIE
    if (pt_on) {                       /* the windows searched, from the samples asked for, at this model's stride */
        char why[256];
        if (0 != flappie_polytail_params(&pt_o, (int)ffhip_model_stride(mdl), &pt_params, why, sizeof why)) { stop_reader_procs(); errx(EXIT_FAILURE, "%s", why); }
    }
    if (bc_kit && NULL == (bc_dev = ffhip_barcodes_upload(eng, bc_kit->n, (const char *const *)bc_kit->seq, args.bc_window))) {
        stop_reader_procs();
        errx(EXIT_FAILURE, "--barcodes: %s", ffhip_last_error());
    }
    if (ad_kit && NULL == (ad_dev = ffhip_adapters_upload(eng, ad_kit->n, (const char *const *)ad_kit->seq))) {
        stop_reader_procs();
        errx(EXIT_FAILURE, "--adapters: %s", ffhip_last_error());
    }
    if (mp_ref && NULL == (mp_dev = ffhip_map_ref_upload(eng, mp_ref->n, (const char *const *)mp_ref->seq))) {
        stop_reader_procs();
        errx(EXIT_FAILURE, "--map: %s", ffhip_last_error());
    }
    if (pu_out && NULL == (pu_dev = ffhip_pileup_create(eng, mp_dev, pu_min_identity))) {
        stop_reader_procs();
        errx(EXIT_FAILURE, "--map-pileup: %s", ffhip_last_error());
    }
    if (mm_out && NULL == (mm_dev = ffhip_modpileup_create(eng, mp_dev, mm_min_identity, mm_lo, mm_hi))) {
        stop_reader_procs();
        errx(EXIT_FAILURE, "--map-mods: %s", ffhip_last_error());
    }
    if (cs_out && NULL == (cs_dev = ffhip_consensus_create(eng, mp_dev, cs_min_identity))) {
        stop_reader_procs();
        errx(EXIT_FAILURE, "--map-consensus: %s", ffhip_last_error());
    }
    if (ep_out && NULL == (ep_dev = ffhip_errprofile_create(eng, ep_min_identity))) {
        stop_reader_procs();
        errx(EXIT_FAILURE, "--truth-errors: %s", ffhip_last_error());
    }
#endif
    hid_t hdf5out = open_or_create_hdf5(args.trace);
    reader_state rs;
    memset(&rs, 0, sizeof(rs));
    in.fl = &fl;                 /* (before the reader thread starts: next_item reads the list through it) */
    /* reads per batch = what one layer launch takes (ffhip_rnn_split.hip): 1024 at H = 256 (the packed forms), 512 at H <= 384 (the dense
     * form), else 256 */
    if (0 == args.batch) args.batch = (int)ffhip_model_launch_reads(mdl);
    if (args.batch <= 0) args.batch = 256;              /* (the query answered 0: no model; never an empty batch) */
    rs.chunk_cap = CHUNK_BATCHES * args.batch;
    g_pack_window = pack_allowed(mdl);
    rs_chunk_cap = (g_pack_window ? PACK_WINDOW_READS : 1) * rs.chunk_cap;      /* reads a chunk may hold (a packed batch takes as many) */
    for (int k = 0; k < NCHUNKBUF; k++) {
        rs.items[k] = calloc(rs_chunk_cap, sizeof(item));
        sem_init(&rs.filled[k], 0, 0);
        sem_init(&rs.empty[k], 0, 1);
    }
    const int threaded = !cli_dbg("no_reader_thread");
    pthread_t reader;
    if (threaded && fl.n > 0 && 0 != pthread_create(&reader, NULL, reader_main, &rs)) errx(EXIT_FAILURE, "could not start the reader thread");
    int first_chunk = 1, last_chunk = (0 == fl.n);
    double t_wait = 0.0;
    if (threaded) { pipe_state.released = release_buffer; pipe_state.released_arg = &rs; }
    /* A LARGE chunk that follows (the window of a directory of long reads: 48 M raw samples and more, what ffhip_prep_create holds behind the engine's last layer launch) has its
     * device pass begun before this chunk's batches are submitted, if the reader has it ready by then (FLAPPIE_DEBUG=no_prep_ahead: never) */
    la.rs = &rs; la.on = threaded && !cli_dbg("no_prep_ahead"); la.taken = 0;
    for (int k = 0; !last_chunk; k = (k + 1) % NCHUNKBUF) {
        const double tw0 = now_s();
        /* buffer k was released when the chunk three back was written: at most two chunks are unfinished at a time (three with a chunk prepared ahead) */
        if (threaded) { if (!la.taken) sem_wait(&rs.filled[k]); }
        else { pipe_wait_slot_written(); read_chunk(first_chunk ? rs.chunk_cap / CHUNK_BATCHES : rs.chunk_cap, rs.items[k], &rs.nitem[k], &rs.last[k]); }
        first_chunk = 0;
        t_wait += now_s() - tw0;
        const int nk = rs.nitem[k];              /* (the reader may refill the buffer as soon as the chunk is written) */
        last_chunk = rs.last[k];
        la.taken = 0; la.kn = (k + 1) % NCHUNKBUF; la.more = !last_chunk;
        if (nk > 0) pipe_chunk(eng, mdl, rs.items[k], nk, k, hdf5out, look_ahead_reader);      /* (no read: the empty last chunk read_chunk describes, or files whose readers died before their first) */
    }
    pipe_drain(mdl, hdf5out);
    if (threaded && fl.n > 0) pthread_join(reader, NULL);
    stop_reader_procs();
    for (int k = 0; k < NCHUNKBUF; k++) free(rs.items[k]);
    for (size_t f = 0; f < fl.n; f++) free(fl.path[f]);      /* (an item holds a copy of its file's name: a file may give thousands of items) */
    free(fl.path);
    if (hdf5out >= 0) { pthread_mutex_lock(&hdf5_lock); H5Fclose(hdf5out); pthread_mutex_unlock(&hdf5_lock); }
    if (stdout != args.output) fclose(args.output);
    for (int k = 0; k < NINFLIGHT; k++) if (batch_cache[k].b) ffhip_batch_destroy(batch_cache[k].b);
    for (int k = 0; k < NINFLIGHT; k++) if (pack_cache[k].b) ffhip_batch_destroy(pack_cache[k].b);
    if (getenv("FLAPPIE_CLI_TIMING")) {
        for (int k = 0; k < 8; k++) fprintf(stderr, "%-24s %8.3f s\n", phase_name[k], t_phase[k]);
        fprintf(stderr, "%-24s %8.3f s\n%-24s %8.3f s\n%-24s %8.3f s\n", "list files", t_listed - t_start, "waiting for the reader", t_wait,
                "files listed -> done", now_s() - t_listed);
        fprintf(stderr, "basecalled: %llu reads, %llu samples (trimmed ranges), %llu raw samples\n", n_called_reads, n_called_samples, n_raw_samples);
        if (n_batches) fprintf(stderr, "batches: %llu (%llu of them packed), %.1f reads each; padding efficiency %.3f by batch (samples / (slots x the batch's longest read, or row)), %.3f by read tile\n", n_batches, n_packed_batches,
                               (double)n_called_reads / (double)n_batches, (double)n_batch_samples / (double)(n_batch_slot_samples ? n_batch_slot_samples : 1),
                               (double)n_batch_samples / (double)(n_tile_slot_samples ? n_tile_slot_samples : 1));
    }
    /* reads with a sample so far out that the default path's operand format could not hold the convolution's output: none is returned
     * clamped, the engine ran them again on its f32 kernels (include/ffhip.h, ffhip_engine_f32_reruns) */
    if (ffhip_engine_f32_reruns(eng) > 0)
        warnx("%llu read(s) held samples beyond the range of the default kernels' operand format and were evaluated on the f32 kernels", ffhip_engine_f32_reruns(eng));
#ifndef BUILD_RUNNIE
    if (bc_kit) {                      /* reads per barcode, then the unclassified ones */
        for (int k = 0; k < bc_kit->n; k++) fprintf(stderr, "barcode\t%s\t%llu\n", bc_kit->name[k], bc_count[k]);
        fprintf(stderr, "barcode\tunclassified\t%llu\n", bc_count[bc_kit->n]);
        ffhip_barcodes_free(bc_dev);
        flappie_barcode_kit_free(bc_kit);
    }
    if (ad_kit) {                      /* kept hits per adapter, reads with a hit, and what --split-reads did */
        for (int k = 0; k < ad_kit->n; k++) fprintf(stderr, "adapter\t%s\t%llu\n", ad_kit->name[k], ad_count[k]);
        fprintf(stderr, "adapters\treads_with_hit\t%llu\nadapters\tsplit_reads\t%llu\nadapters\tpieces\t%llu\nadapters\tdropped_pieces\t%llu\nadapters\toverflow\t%llu\n",
                ad_reads_with_hit, ad_stats[0], ad_stats[1], ad_stats[2], ad_stats[3]);
        ffhip_adapters_free(ad_dev);
        flappie_adapter_kit_free(ad_kit);
    }
    if (pu_dev) {                      /* the table, once: every batch object is gone, so every accumulation is done; reads counted and skipped, positions, those covered, the ops */
        const size_t P = ffhip_pileup_positions(pu_dev);
        uint32_t *counts = malloc((P ? P : 1) * FFHIP_PILEUP_PLANES * sizeof *counts);
        ffhip_pileup_totals tot;
        unsigned long long covered = 0;
        if (NULL == counts || 0 != ffhip_pileup_download(pu_dev, counts, &tot)) warnx("--map-pileup: %s", counts ? ffhip_last_error() : "out of memory for the table");
        else {
            flappie_pileup_write(pu_out, mp_ref, counts, &covered);
            flappie_pileup_summary_print(stderr, &tot, (unsigned long long)P, covered);
        }
        free(counts);
        if (0 != fclose(pu_out)) warnx("--map-pileup %s: write failed", pu_path);
        ffhip_pileup_free(pu_dev);
    }
    if (mm_dev) {                      /* the bedMethyl table and the histogram, once: every batch object is gone, so every accumulation is done */
        const size_t P = ffhip_modpileup_positions(mm_dev);
        uint32_t *counts = malloc((P ? P : 1) * FFHIP_MODPILEUP_PLANES * sizeof *counts);
        ffhip_modpileup_totals tot;
        uint64_t hist[256];
        unsigned long long rows = 0;
        if (NULL == counts || 0 != ffhip_modpileup_download(mm_dev, counts, &tot, hist)) warnx("--map-mods: %s", counts ? ffhip_last_error() : "out of memory for the table");
        else {
            flappie_modpileup_write(mm_out, mp_ref, counts, (mm_motif && 0 == strcmp(mm_motif, "C")) ? FLAPPIE_MODS_MOTIF_C : FLAPPIE_MODS_MOTIF_CG, mm_combine, &rows);
            if (mm_hist) flappie_modpileup_hist_write(mm_hist, hist);
            flappie_modpileup_summary_print(stderr, &tot, rows);
        }
        free(counts);
        if (0 != fclose(mm_out)) warnx("--map-mods %s: write failed", mm_path);
        if (mm_hist && 0 != fclose(mm_hist)) warnx("--map-mods-hist %s: write failed", mm_hist_path);
        ffhip_modpileup_free(mm_dev);
    }
    if (cs_dev) {                      /* the consensus, called once: every batch object is gone, so every accumulation is done; the planes come down for the changes only */
        const size_t P = ffhip_consensus_positions(cs_dev);
        ffhip_consensus_cell *cells = malloc((P ? P : 1) * sizeof *cells);
        uint32_t *counts = cs_changes ? malloc((P ? P : 1) * FFHIP_CONSENSUS_PLANES * sizeof *counts) : NULL;
        ffhip_consensus_totals tot;
        flappie_consensus_stats st;
        if (NULL == cells || (cs_changes && NULL == counts)) warnx("--map-consensus: out of memory for the cells");
        else if (0 != ffhip_consensus_call(cs_dev, cs_min_depth, cells) || 0 != ffhip_consensus_download(cs_dev, counts, &tot)) warnx("--map-consensus: %s", ffhip_last_error());
        else {
            flappie_consensus_write(cs_out, mp_ref, cells, &st);
            if (cs_changes) flappie_consensus_changes_write(cs_changes, mp_ref, cells, counts);
            flappie_consensus_summary_print(stderr, &tot, &st);
        }
        free(counts);
        free(cells);
        if (0 != fclose(cs_out)) warnx("--map-consensus %s: write failed", cs_path);
        if (cs_changes && 0 != fclose(cs_changes)) warnx("--map-consensus-changes %s: write failed", cs_changes_path);
        ffhip_consensus_free(cs_dev);
    }
    if (ep_dev) {                      /* the error profile, once: every batch object is gone, so every accumulation is done */
        uint64_t *counts = malloc(FFHIP_ERRPROFILE_TABLE_WORDS * sizeof *counts);
        ffhip_errprofile_totals tot;
        if (NULL == counts) warnx("--truth-errors: out of memory for the counters");
        else if (0 != ffhip_errprofile_download(ep_dev, counts, &tot)) warnx("--truth-errors: %s", ffhip_last_error());
        else {
            flappie_errprofile_write(ep_out, counts);
            flappie_errprofile_summary_print(stderr, &tot);
        }
        free(counts);
        if (0 != fclose(ep_out)) warnx("--truth-errors %s: write failed", ep_path);
        ffhip_errprofile_free(ep_dev);
    }
    if (mp_ref) {                      /* reads, mapped, unmapped, discordant; the mapped reads' anchor distances over their anchor bases */
        flappie_map_summary_print(stderr, &mp_sum);
        if (0 != fclose(mp_out)) warnx("--map-out %s: write failed", map_out_path);
        if (mp_recs && 0 != fclose(mp_recs)) warnx("--map-records %s: write failed", map_recs_path);
        ffhip_map_ref_free(mp_dev);
        flappie_map_ref_free(mp_ref);
    }
    if (pt_on) {                      /* reads with a record, with a tail and a rate, with a tail alone; the median tail */
        flappie_polytail_summary_print(stderr, &pt_sum);
        flappie_polytail_summary_free(&pt_sum);
    }
    if (rm_refs || rfm_on) {           /* mapped, no record (--remap-from-map: not placed by the map), refused, and the mapped reads whose path touched the band */
        fprintf(stderr, "remap\tmapped\t%llu\nremap\tno_record\t%llu\nremap\trefused\t%llu\nremap\tband_touched\t%llu\n", rm_count[0], rm_count[1], rm_count[2], rm_count[3]);
        if (0 != fclose(rm_out)) warnx("--remap-out %s: write failed", args.remap_out);
        if (ev_out) {                  /* mapped reads written, and their bases */
            fprintf(stderr, "events\treads\t%llu\nevents\tbases\t%llu\n", ev_count[0], ev_count[1]);
            if (0 != fclose(ev_out)) warnx("--remap-events %s: write failed", args.remap_events);
        }
        if (md_out) {                  /* mapped reads written, and their sites */
            fprintf(stderr, "mods\treads\t%llu\nmods\tsites\t%llu\n", md_count[0], md_count[1]);
            if (0 != fclose(md_out)) warnx("--remap-mods %s: write failed", mods_path);
        }
        if (vr_out) {                  /* mapped reads written, their variants, the file's lines that were skipped, and the variants of records no mapped read had */
            unsigned long long skipped = 0, unmapped = 0;
            for (int k = 0; k < FLAPPIE_VARIANTS_KINDS; k++) skipped += vr_vars->skipped[k];
            for (int k = 0; k < rm_refs->n; k++) if (!vr_done[k]) unmapped += flappie_variants_of(vr_vars, k, NULL);
            fprintf(stderr, "variants\treads\t%llu\nvariants\tscored\t%llu\nvariants\tskipped\t%llu\nvariants\tunmapped\t%llu\n", vr_count[0], vr_count[1], skipped, unmapped);
            if (0 != fclose(vr_out)) warnx("--remap-variants-out %s: write failed", vars_out_path);
            flappie_variants_free(vr_vars);
            free(vr_done);
        }
        flappie_remap_refs_free(rm_refs);
    }
    if (tr_refs) {                     /* reads aligned, not aligned, without a record, the pooled and the median identity */
        flappie_truth_summary_print(stderr, &tr_sum);
        flappie_truth_summary_free(&tr_sum);
        if (0 != fclose(tr_out)) warnx("--truth-out %s: write failed", args.truth_out);
        flappie_remap_refs_free(tr_refs);
    }
    if (tfm_on) {                      /* the same lines: the reads that were not mapped count as no_record */
        flappie_truth_summary_print(stderr, &tr_sum);
        flappie_truth_summary_free(&tr_sum);
        if (0 != fclose(tr_out)) warnx("--truth-out %s: write failed", args.truth_out);
        if (tfm_sam && 0 != fclose(tfm_sam)) warnx("--map-sam %s: write failed", tfm_sam_path);
    }
#endif
    flappie_hip_shutdown();
    if (reader_failures) { warnx("%d reader process(es) failed; see the warnings above", reader_failures); return EXIT_FAILURE; }
    if (n_lost_reads > 0) { warnx("%llu read(s) were not called: their batches failed (see the warnings above)", n_lost_reads); return EXIT_FAILURE; }
    return EXIT_SUCCESS;
}

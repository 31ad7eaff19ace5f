"""The move table and signal tags of `flappie --emit-moves` restated in plain Python (include/ffhip.h FFHIP_RUN_MOVES, include/flappie_moves.h).

For a read of nblock blocks with the Viterbi path path[0 .. nblock]:
    positions = every pos in [1, nblock) with path[pos] != path[pos - 1]          (the reference's change_positions, decode.c:66-79)
    move[b]   = 1 iff b + 1 is a position, i.e. 0 <= b <= nblock - 2 and path[b + 1] != path[b];  move[nblock - 1] = 0
Block b stands for the samples [start + b * stride, start + (b + 1) * stride) of the raw signal, clipped to the read's end.  A record's tags, in this order:
    qs:f: mean quality (absent for an empty call), ns:i: samples in the file, ts:i: start + stride * (first block with a move),
    sm:f: sd:f: sv:Z:med_mad (absent under --delta), mv:B:c, stride, then the moves from the first 1 on.
mv is in signal order whatever the orientation of SEQ."""
import math

import numpy as np

import modbase_ref as MR

LETTERS = "ACGTZ"


def positions(path):
    """change positions of a path of nblock + 1 entries: pos in [1, nblock) with a new state"""
    nblock = len(path) - 1
    return [pos for pos in range(1, nblock) if int(path[pos]) != int(path[pos - 1])]


def moves(path):
    nblock = len(path) - 1
    mv = np.zeros(nblock, dtype=np.uint8)
    for pos in positions(path):
        mv[pos - 1] = 1
    return mv


def call_through_moves(path, mv, nbase):
    """the call re-read through the moves: the state entered by every block with a move"""
    return "".join(LETTERS[int(path[b + 1]) % nbase] for b in range(len(mv)) if mv[b])


def mean_quality(qual):
    """-10 log10( mean_i 10^(-(Q_i - 33) / 10) ), summed in the string's order"""
    total = 0.0
    for c in qual:
        total += 10.0 ** (-(float(ord(c)) - 33.0) / 10.0)
    return -10.0 * math.log10(total / float(len(qual))) + 0.0


def first_move(mv):
    nz = np.flatnonzero(np.asarray(mv))
    return int(nz[0]) if nz.size else None


def tags(mv, stride, n, start, qual, median, mad, delta):
    """the tag text of one record: the list of its tab-separated fields"""
    out = []
    if qual:
        out.append("qs:f:%.3f" % mean_quality(qual))
    b0 = first_move(mv)
    out.append("ns:i:%d" % n)
    out.append("ts:i:%d" % (start + stride * (b0 if b0 is not None else 0)))
    if not delta:
        out += ["sm:f:%.9g" % float(np.float32(median)), "sd:f:%.9g" % float(np.float32(mad)), "sv:Z:med_mad"]
    kept = [] if b0 is None else [int(v) for v in np.asarray(mv)[b0:]]
    out.append("mv:B:c,%d" % stride + "".join(",%d" % v for v in kept))
    return out


def parse_mv(tag):
    assert tag.startswith("mv:B:c,")
    v = [int(x) for x in tag[len("mv:B:c,"):].split(",")]
    return v[0], v[1:]


def base_samples(ts, stride, mv):
    """from (ts, stride, mv) alone: [first, last) samples of every base -- from its move's block to the next base's (the last base: to the end of mv)"""
    ones = [k for k, v in enumerate(mv) if v]
    ends = ones[1:] + [len(mv)]
    return [(ts + stride * a, ts + stride * e) for a, e in zip(ones, ends)]


def oriented(call, qual, ml, reverse):
    """--reverse: the call, its qualities and its ML bytes (None: none) reversed together; the moves stay in signal order"""
    ml = None if ml is None else list(ml)
    if reverse:
        return call[::-1], qual[::-1], None if ml is None else ml[::-1]
    return call, qual, ml


def _tail(seq_call, mv, stride, n, start, qual, median, mad, delta, ml):
    fields = []
    seq = seq_call
    if ml is not None:
        seq = MR.seq_of(seq_call)
        fields += list(MR.tags(seq, ml))
    fields += tags(mv, stride, n, start, qual, median, mad, delta)
    return seq, "\t".join(fields)


def tagged_fastq(header, call, qual, mv, stride, n, start, median, mad, delta, ml=None):
    """a default FASTQ record (header line without '@' and newline) -> the --emit-moves record (with MM / ML in front when ml is given)"""
    seq, tail = _tail(call, mv, stride, n, start, qual, median, mad, delta, ml)
    return "@%s\t%s\n%s\n+\n%s\n" % (header, tail, seq, qual)


def tagged_fasta(header, call, qual, mv, stride, n, start, median, mad, delta, ml=None):
    seq, tail = _tail(call, mv, stride, n, start, qual, median, mad, delta, ml)
    return ">%s\t%s\n%s\n" % (header, tail, seq)


def tagged_sam(qname, call, qual, mv, stride, n, start, median, mad, delta, ml=None):
    seq, tail = _tail(call, mv, stride, n, start, qual, median, mad, delta, ml)
    return "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\t%s\n" % (qname, seq, qual, tail)

"""The 5mC reporting of `flappie --modbase-tags` restated in numpy fp64 (include/ffhip.h FFHIP_RUN_MOD_PROBS, include/flappie_modbase.h).

A called base is a change position pos (1 <= pos < nblock, path[pos] != path[pos - 1]), as k_assemble and the reference define it.  A called C or Z
(state % 5 == 1 or 4) gets, with x = exp(L[pos - 1]) of the log posterior L [nblock][60],
    occ(j) = sum_{f<10} x[10 j + f] + x[50 + j] + x[55 + j]
    p      = occ(4) / (occ(1) + occ(4))          (0 if the denominator is 0 or not finite)
    ML     = min(255, floor(256 p))              (SAMv1 1.7: N stands for [N/256, (N+1)/256))
Every other called base gets 0.  A record's SEQ is the call with Z written as C; MM:Z:C+m? lists every C of SEQ with skip 0, ML:B:C their bytes."""
import numpy as np

NBASE, NS, OFF = 5, 10, 50
LETTERS = "ACGTZ"


def called(path, nblock=None):
    """positions of the called bases of a path (its first nblock entries)"""
    path = np.asarray(path)
    n = len(path) if nblock is None else nblock
    return [p for p in range(1, n) if path[p] != path[p - 1]]


def occupancy(row, j):
    x = np.exp(np.asarray(row, dtype=np.float64))
    return float(x[NS * j:NS * j + NS].sum() + x[OFF + j] + x[OFF + NBASE + j])


def p_mod(row):
    c, z = occupancy(row, 1), occupancy(row, 4)
    den = c + z
    if not (den > 0.0 and np.isfinite(den)):
        return 0.0
    return z / den


def ml_byte(p):
    return int(min(255, np.floor(256.0 * p)))


def mod_probs(path, logpost):
    """(bytes, 256 p) of every called base: bytes as the device makes them, 256 p in fp64 (NaN for A, G, T)"""
    logpost = np.asarray(logpost)
    out, raw = [], []
    for pos in called(path, logpost.shape[0]):
        if int(path[pos]) % NBASE in (1, 4):
            p = p_mod(logpost[pos - 1])
            out.append(ml_byte(p))
            raw.append(256.0 * p)
        else:
            out.append(0)
            raw.append(np.nan)
    return np.array(out, dtype=np.uint8), np.array(raw, dtype=np.float64)


def basecall(path, nblock=None):
    return "".join(LETTERS[int(path[p]) % NBASE] for p in called(path, nblock))


def seq_of(call):
    return call.replace("Z", "C")


def tags(seq, ml):
    """(MM tag, ML tag) of a SEQ (no Z) and its bytes, one per base of seq"""
    idx = [i for i, c in enumerate(seq) if c == "C"]
    mm = "MM:Z:C+m?" + "".join(",0" for _ in idx) + ";"
    mlt = "ML:B:C" + "".join(",%d" % int(ml[i]) for i in idx)
    return mm, mlt


def oriented(call, qual, ml, reverse):
    """--reverse applies first: the call, its qualities and its bytes reversed together"""
    if reverse:
        return call[::-1], qual[::-1], list(ml)[::-1]
    return call, qual, list(ml)


def tagged_fastq(header, call, qual, ml):
    """a default FASTQ record (header line without '@' and newline) -> the --modbase-tags record"""
    seq = seq_of(call)
    mm, mlt = tags(seq, ml)
    return "@%s\t%s\t%s\n%s\n+\n%s\n" % (header, mm, mlt, seq, qual)


def tagged_fasta(header, call, ml):
    seq = seq_of(call)
    mm, mlt = tags(seq, ml)
    return ">%s\t%s\t%s\n%s\n" % (header, mm, mlt, seq)


def tagged_sam(qname, call, qual, ml):
    seq = seq_of(call)
    mm, mlt = tags(seq, ml)
    return "%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\t%s\t%s\n" % (qname, seq, qual, mm, mlt)


def ml_values(ml_tag):
    assert ml_tag.startswith("ML:B:C")
    rest = ml_tag[len("ML:B:C"):]
    return [int(v) for v in rest.split(",")[1:]] if rest else []


def spread_ml(seq, values):
    """the bytes of a SEQ's Cs put back at their bases (0 elsewhere)"""
    out = [0] * len(seq)
    it = iter(values)
    for i, c in enumerate(seq):
        if c == "C":
            out[i] = next(it)
    return out

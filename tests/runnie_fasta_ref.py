"""Restatements for runnie's FASTA mode (tests/test_runnie_fasta.py, tests/test_runnie_fasta_gpu.py), in numpy:

  records(path, mat, nbase)   runnie.c:282-313: the run records (base, shape, scale, dwell) of a decoded read
  run_text(name, recs)        the .run text runnie writes for them (`# name`, then base<TAB>%f<TAB>%f<TAB>dwell)
  fasta_from_run(text, ...)   decode_runnie.py on such a text: its stdout and stderr (run_estimate_modes on the PARSED six-decimal scale, 60 a line)
  estimate(base, scale, f)    the device's form of the same estimate on fp32 scales: max(1, floor(rint(scale * 1e6) / 1e6 * f[base]))
  fasta_record(name, bases, est, rlc)   one read's FASTA text from its runs (None: no basecall)"""
import numpy as np

ALPHABET = "ACGT"
DEFAULT = (1.02, 1.04, 1.04, 1.02)


def records(path, mat, nbase=4):
    """path: at least nblock entries, mat: [nblock][nparam] (posterior, or transitions under --viterbi)"""
    nblock = mat.shape[0]
    out, last, dwell = [], -1, 1
    for blk in range(nblock + 1):
        emit = (path[blk] < nbase) if blk < nblock else True
        if not emit:
            dwell += 1
            continue
        if last >= 0:
            b = int(path[last])
            out.append((b, np.float32(mat[last, b]), np.float32(mat[last, nbase + b]), dwell))
        last, dwell = blk, 1
    return out


def run_text(name, recs):
    return "# %s\n" % name + "".join("%s\t%f\t%f\t%d\n" % (ALPHABET[b], sh, sc, d) for b, sh, sc, d in recs)


def _wrap(seq, width=60):
    return "\n".join(seq[st:st + width] for st in range(0, len(seq), width)) + "\n"


def fasta_from_run(text, factors=DEFAULT, rlc=False):
    """(stdout, stderr) of decode_runnie.py [--rlc] [--scale ...] reading `text`"""
    reads, name, data = [], None, None
    for line in text.splitlines(keepends=True):
        if line.startswith("#"):
            if name is not None:
                reads.append((name, data))
            name, data = line[2:-1], []
        else:
            data.append(line.split("\t"))
    if name is not None:
        reads.append((name, data))
    out, err = [], []
    f = np.array(factors, dtype=np.float64)
    for name, data in reads:
        if rlc:
            seq = "".join(d[0] for d in data)
        elif not data:
            seq = None
        else:
            bases = np.array([ALPHABET.index(d[0]) for d in data])
            scale = np.array([float(d[2]) for d in data])
            est = np.maximum(1, np.floor(scale * f[bases])).astype(np.int64)
            seq = "".join(ALPHABET[b] * int(r) for b, r in zip(bases, est))
        if seq is None:
            err.append("No basecall returned for %s\n" % name)
        else:
            out.append(">%s\n%s" % (name, _wrap(seq)))
    return "".join(out), "".join(err)


def estimate(base, scale, factors=DEFAULT):
    """per run: the estimate, and whether the read fails (non-finite scale, estimate >= 2^31)"""
    scale = np.asarray(scale, dtype=np.float32).astype(np.float64)
    f = np.array(factors, dtype=np.float64)[np.asarray(base, dtype=np.int64)]
    with np.errstate(all="ignore"):
        e = np.floor(np.rint(scale * 1e6) / 1e6 * f)
        bad = ~np.isfinite(scale) | ~(e < 2.0 ** 31)
        est = np.where(bad, 0, np.maximum(1, np.where(bad, 0, e))).astype(np.int64)
    return est, bool(bad.any())


def fasta_record(name, bases, est, rlc=False):
    bases = np.asarray(bases, dtype=np.int64)
    if rlc:
        return ">%s\n%s" % (name, _wrap("".join(ALPHABET[b] for b in bases)))
    if bases.size == 0:
        return None
    return ">%s\n%s" % (name, _wrap("".join(ALPHABET[b] * int(r) for b, r in zip(bases, est))))

"""Restatement of "remap from map" (include/ffhip.h) in plain python integers, on top of map_ref.py, maptruth_ref.py and remap_ref.py.

  stretch of a map record with status 1, search q = 2 k + o, span [tstart, tend):  y_q[tstart : tend] as codes 0 .. 3, m = tend - tstart bases, in signal order
  coding:  q_i = s_i + nbase ((i - runstart_i) & 1), runstart_i the first position of the run of equal letters that i lies in
  entry i:  trans_lookup(q_i, q_i) | trans_lookup(q_{i-1}, q_i) << 8, the high byte 0 at i = 0
  the rule, room = N + 1 for a read of N >= 1 blocks:
      map status 1, 1 <= m <= room:  remap status 1, L = m, the entries
      map status 1, m > room:        remap status 2, L = m, nothing coded
      map status 0, 2 or 3:          remap status 0, L = 0

and of the host side: the line of map.tsv in the mode, and the reference the GPU tests build from a batch's own calls."""
import numpy as np

import map_ref as R
import maptruth_ref as MT
import remap_ref as RR


def run_parity_code(s, nbase):
    """the coding without the recurrence: a position's parity inside its run of equal letters"""
    q, start = [], 0
    for i, x in enumerate(s):
        if i == 0 or int(x) != int(s[i - 1]):
            start = i
        q.append(int(x) + nbase * ((i - start) & 1))
    return q


def entries(s, nbase):
    """what the device holds for a sequence of codes: uint16 [L], stay | move << 8"""
    q = run_parity_code(s, nbase)
    return np.array([RR.trans_lookup(q[i], q[i], nbase) | ((RR.trans_lookup(q[i - 1], q[i], nbase) if i else 0) << 8) for i in range(len(q))], np.uint16)


def entries_by_remap_ref(s, nbase):
    """the same from remap_ref's own coding (the recurrence)"""
    q = RR.flipflop_code(s, nbase)
    return np.array([RR.trans_lookup(q[i], q[i], nbase) | ((RR.trans_lookup(q[i - 1], q[i], nbase) if i else 0) << 8) for i in range(len(q))], np.uint16)


def remap_from_map(records, mp: dict, nblock: int, nbase: int):
    """(status, L, entries or None) of a read of nblock >= 1 blocks whose map record is mp"""
    if mp["status"] != 1:
        return 0, 0, None
    s = MT.stretch(records, mp["q"], mp["tstart"], mp["tend"])
    m = int(s.size)
    assert m >= 1
    if m > nblock + 1:
        return 2, m, None
    return 1, m, entries(s, nbase)


def sequence_of(records, mp: dict):
    """the codes a second run is given for this read through ffhip_batch_set_remap: the stretch, None unless the record says mapped"""
    return MT.stretch(records, mp["q"], mp["tstart"], mp["tend"]) if mp["status"] == 1 else None


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def reference_of(rng, calls):
    """random flanks and the reads' own calls in three records: five in six of them, two in three of those with 5 % edits, on alternating strands (the construction
    of the tests of truth from map, restated)"""
    recs = ["", "", ""]
    for i, c in enumerate(calls):
        if not c or i % 6 == 5:
            continue                                          # left out: this read does not map
        x = c.replace("Z", "C")
        if i % 3:
            x = R.edit(rng, x, 0.05)
        recs[i % 3] += rand_seq(rng, 150 + 37 * (i % 5)) + (x if i % 2 == 0 else R.revcomp(x))
    return [r + rand_seq(rng, 200) for r in recs]


def tally(maps, remaps):
    """what keeps a batch test from passing empty, from the reads' map and remap records"""
    seen = {"reads": 0, "mapped": 0, "plus": 0, "minus": 0, "not mapped": 0}
    for mp, rm in zip(maps, remaps):
        ok = mp["status"] == 1 and rm["status"] == 1
        seen["reads"] += 1
        seen["mapped"] += ok
        seen["plus"] += ok and not mp["q"] & 1
        seen["minus"] += ok and mp["q"] & 1
        seen["not mapped"] += mp["status"] != 1
    return seen


def tally_ok(seen):
    return seen["mapped"] * 4 >= seen["reads"] * 3 and seen["plus"] >= 2 and seen["minus"] >= 2 and seen["not mapped"] >= 1


# ---- the host side
def map_tsv_line(name: str, rm: dict, stride: int, trim_start: int, band: int, mp: dict, names, lens) -> str:
    """the line of map.tsv in the mode: the columns of --remap-out (name, status, nblock, stride, trim_start, L, band, maxdev, score as %.9g, the starts; * for the
    last three unless status is 1), then record, strand, tstart, tend as hits.tsv has them"""
    k, o, a, b = R.forward(mp["q"], mp["tstart"], mp["tend"], lens)
    head = "%s\t%d\t%d\t%d\t%d\t%d\t%d\t" % (name, rm["status"], rm["nblock"], stride, trim_start, rm["L"], band)
    if rm["status"] == 1:
        starts, maxdev = RR.starts_maxdev(rm["rm"], rm["L"])
        head += "%d\t%s\t%s" % (maxdev, c_g9(rm["score"]), ",".join(str(int(x)) for x in starts))
    else:
        head += "*\t*\t*"
    return head + "\t%s\t%s\t%d\t%d\n" % (names[k], o, a, b)


def c_g9(x) -> str:
    """C's %.9g of a float32 promoted to double"""
    return "%.9g" % float(np.float32(x))

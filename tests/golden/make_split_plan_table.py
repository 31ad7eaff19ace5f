#!/usr/bin/env python3
"""tests/golden/split_plan_table.json: what a layer launch of the split-operand kernels looks like for every (kind, H, ncu, FFHIP_DEBUG, beside, remaining) of
tests/test_split_plan.py, recorded from the rules of the commit BEFORE split_plan replaced them (1090c9f): that commit's release library, its
ffhip::split_next_launch_tiles, split_launch_workgroups, split_workgroups_per_cu and split_pair_ok called through ctypes by their mangled names.

This script runs ONLY against that parent's library: the tree that holds it no longer has those four symbols (one function, split_plan, took their place; the
test reads it through ffhip_debug_split_plan).  It needs no GPU.
usage: tests/golden/make_split_plan_table.py PARENT/flappie_amd/libffhip.so [OUT.json]

Per row, for remaining = 1, 2, ...: [nrt, ts, workgroups, per_cu, fills_chip, pair_ok, pair_ok under no_pair], equal neighbours run-length coded as [count, [...]].
 - fills_chip is the expression the parent's engine wrote out at its two call sites: 2 * workgroups > ncu * per_cu.
 - ts (tiles a group) was a static function there.  It is recorded as what the parent's grid says: 1 where workgroups == 32 nrt, 2 where workgroups == 32 ceil(nrt / 2)
   or 16 (nrt / 2) (the packed forms' groups hold a pair of tiles too), and 0 -- not observable -- for a launch of ONE tile, whose grid is 32 either way.
 - the form was not observable at all; the test ties it to these values instead."""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS, HS, NCUS, BESIDE = (0, 1), (128, 256, 384, 512), (16, 32, 64, 256, 304), (0, 1)
DEBUGS = ("", "no_dense", "no_pack", "no_dense,no_pack")


def max_remaining(ncu):          # past the largest full launch (8 tiles a unit of 32 compute units: the packed forms)
    return 8 * max(1, ncu // 32) + 2


def set_debug(tokens):
    if tokens:
        os.environ["FFHIP_DEBUG"] = tokens
    else:
        os.environ.pop("FFHIP_DEBUG", None)


def rle(rows):
    out = []
    for r in rows:
        if out and out[-1][1] == r:
            out[-1][0] += 1
        else:
            out.append([1, r])
    return out


def main():
    L = C.CDLL(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "split_plan_table.json")
    nxt, wgs, pcu, pair = (getattr(L, n) for n in ("_ZN5ffhip23split_next_launch_tilesEiiii", "_ZN5ffhip23split_launch_workgroupsEiiiii",
                                                   "_ZN5ffhip23split_workgroups_per_cuEiiiii", "_ZN5ffhip13split_pair_okEiiii"))
    pair.restype = C.c_bool
    table = {}
    for kind in KINDS:
        for H in HS:
            for ncu in NCUS:
                for dbg in DEBUGS:
                    for beside in BESIDE:
                        rows = []
                        for remaining in range(1, max_remaining(ncu) + 1):
                            set_debug(dbg)
                            nrt = nxt(kind, H, remaining, ncu)
                            w, p = wgs(kind, H, nrt, ncu, beside), pcu(kind, H, nrt, ncu, beside)
                            ts = 0 if nrt == 1 else (1 if w == 32 * nrt else (2 if w in (32 * ((nrt + 1) // 2), 16 * (nrt // 2)) else -1))
                            assert ts >= 0, (kind, H, ncu, dbg, beside, remaining, nrt, w)
                            ok = int(pair(kind, H, nrt, ncu))
                            set_debug((dbg + "," if dbg else "") + "no_pair")
                            rows.append([nrt, ts, w, p, int(2 * w > ncu * p), ok, int(pair(kind, H, nrt, ncu))])
                        table["%d,%d,%d,%s,%d" % (kind, H, ncu, dbg, beside)] = rle(rows)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
    print("wrote", out, "from", sys.argv[1], len(table), "rows")


if __name__ == "__main__":
    main()

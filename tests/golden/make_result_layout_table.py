#!/usr/bin/env python3
"""tests/golden/result_layout_table.json: every offset of a batch's result block for the grid of tests/test_result_layout.py, from the arithmetic of
res_layout() in flappie_amd/csrc/ffhip_engine.hip of the commit BEFORE the block was described by a table (43c3ad8), restated here line for line in plain
Python.  It loads no library and needs no GPU.
usage: tests/golden/make_result_layout_table.py [OUT.json]

Per case "nread,cap_reads,Tb,sections" the 21 values of that commit's ResLayout, in its order (NAMES).  Only mod_block entered its arithmetic; the other
sections' offsets are the same whether the block holds them or not."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("sat", "abort", "lens", "score", "bases", "quals", "end", "nrun", "fail", "len", "base", "est", "runs_end", "shape", "scale", "dwell", "rec_end",
         "ml", "ml_end", "mv", "mv_end")
NREADS, CAP_FACTORS, TBS = (1, 16, 17, 512), (1, 8), (1, 255, 256, 45670)
# every section set a batch can reach: a run-length batch grows runs, then records; a flip-flop batch mod and moves in either order (mv behind the core or behind ml)
SECTION_SETS = ((), ("runs",), ("runs", "records"), ("mod",), ("moves",), ("mod", "moves"))


def up(x):
    return (x + 255) & ~255


def res_layout(nread, cap_reads, Tb, mod_block):
    Bp = (nread + 15) // 16 * 16
    nres, n1 = cap_reads, nread * (Tb + 1)
    o = {}
    o["sat"] = 0; o["abort"] = up(Bp * 4); o["lens"] = o["abort"] + 256; o["score"] = o["lens"] + up(nres * 4)
    o["bases"] = o["score"] + up(nres * 4); o["quals"] = o["bases"] + up(n1); o["end"] = o["quals"] + up(n1)
    o["nrun"] = o["end"]; o["fail"] = o["nrun"] + up(nres * 4); o["len"] = o["fail"] + up(nres * 4); o["base"] = o["len"] + up(nres * 8); o["est"] = o["base"] + up(n1)
    o["runs_end"] = o["est"] + up(n1 * 4)
    o["shape"] = o["runs_end"]; o["scale"] = o["shape"] + up(n1 * 4); o["dwell"] = o["scale"] + up(n1 * 4); o["rec_end"] = o["dwell"] + up(n1 * 4)
    o["ml"] = o["end"]; o["ml_end"] = o["ml"] + up(n1)
    o["mv"] = o["ml_end"] if mod_block else o["end"]; o["mv_end"] = o["mv"] + up(n1)
    return [o[k] for k in NAMES]


def cases():
    for nread in NREADS:
        for f in CAP_FACTORS:
            for Tb in TBS:
                for secs in SECTION_SETS:
                    yield nread, nread * f, Tb, secs


def key(nread, cap_reads, Tb, secs):
    return "%d,%d,%d,%s" % (nread, cap_reads, Tb, "+".join(secs))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "result_layout_table.json")
    table = {key(n, c, t, s): res_layout(n, c, t, "mod" in s) for n, c, t, s in cases()}
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
    print("wrote", out, len(table), "cases")


if __name__ == "__main__":
    main()

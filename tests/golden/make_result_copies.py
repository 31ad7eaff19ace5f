#!/usr/bin/env python3
"""tests/golden/result_copies.json: what every finished run of the cases below copies to the host and what its batch holds on the device, recorded from the
release library of the commit BEFORE the result block was described by a table (43c3ad8).  tests/test_result_copies_gpu.py runs the same cases (record() below)
on the library of its tree and holds it to these figures exactly.

This script runs in a built checkout of that parent (copied to its tests/golden/: it imports the flappie_amd beside it, whose binding matches that library)
and needs a GPU:
usage: PARENT/tests/golden/make_result_copies.py [OUT.json]

Per case, after each finish of its flag sequence: [device-to-host copy calls, device-to-host bytes (ffhip_copy_counts, reset before the run), device bytes the
batch holds (ffhip_debug_batch_device_bytes), reads run again on the f32 path].  Copies inside the re-run that stay on one side (device to device, host to host)
are not in these counters."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from flappie_amd import binding as B  # noqa: E402
from flappie_amd import model as M  # noqa: E402

NONE, MOVES, MOD, RUNS, RECORDS = 0, B.RUN_MOVES, B.RUN_MOD_PROBS, B.RUN_RLE_RUNS, B.RUN_RLE_RECORDS
# flag sequences that grow the block in every order, per model
SEQUENCES = {
    "lstm5": {"none_moves_none": (NONE, MOVES, NONE),
              "undecoded": (B.RUN_NO_DECODE, NONE, B.RUN_VITERBI_ONLY | MOVES, B.RUN_NO_DECODE)},
    "grumod5": {"none_moves_none": (NONE, MOVES, NONE),
                "mod_moves_mod": (MOD, MOVES, MOD, MOD | MOVES),
                "moves_mod_moves": (MOVES, MOD, MOVES, MOD | MOVES, MOVES, NONE),       # (the last MOVES: moves alone after both exist)
                "undecoded": (B.RUN_NO_DECODE, B.RUN_VITERBI_ONLY | MOD, B.RUN_NO_DECODE, B.RUN_VITERBI_ONLY | MOD | MOVES)},
    "rle": {"runs_records": (RUNS, RECORDS, RUNS, NONE),
            "records_first": (RECORDS, RUNS, NONE, RECORDS),
            "undecoded": (B.RUN_NO_DECODE, RUNS, B.RUN_NO_DECODE)},
}
# a saturating outlier (a sample beyond the split format's range): the f32 re-run runs with each section made.  lstm5mod: the LSTM trunk under the 5-base head
# (the GRUmod trunk's convolution ends in tanh: no sample takes it out of range)
OUTLIER = {"lstm5": (MOVES, NONE), "lstm5mod": (MOD | MOVES, MOD, MOVES), "rle": (RECORDS, RUNS, NONE)}


def models():
    lstm, gru = M.synthetic_model(M.NET_LSTM5, 128, seed=1), M.synthetic_model(M.NET_GRUMOD5, 128, seed=1)
    return {"lstm5": lstm, "grumod5": gru, "rle": M.synthetic_model(M.NET_LSTM5_RLE, 128, seed=1),
            "lstm5mod": M.FlipflopModel(M.NET_LSTM5, lstm.convs, lstm.rnns, gru.FF_W, gru.FF_b)}


def _counts():
    c = (C.c_ulonglong * 5)()
    B.lib().ffhip_copy_counts.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    B.lib().ffhip_copy_counts.restype = None
    B.lib().ffhip_copy_counts(c, 1)
    return int(c[2]), int(c[3])


def _batch(dm, form, outlier):
    """`form` rows: 8 reads of 2000 samples, one a row; packed: 40 reads of mixed lengths in 16 rows.  outlier: one sample of read 1 at 6e4"""
    rng = np.random.default_rng(11)
    if form == "rows":
        sig = rng.standard_normal((8, 2000)).astype(np.float32)
        if outlier:
            sig[1, 200] = 6.0e4
        b = B.Batch(dm, 8, 2000)
        b.set_signals(sig)
        return b
    lens = [int(x) for x in np.clip(np.exp(np.log(300) + 0.8 * rng.standard_normal(40)), 250, 1950)]
    sigs = [rng.standard_normal(n).astype(np.float32) for n in lens]
    if outlier:
        sigs[1][200] = 6.0e4
    b = B.Batch(dm, 16, 2000, max_reads=len(sigs))
    slot, off = b.pack_plan(lens)
    assert min(slot) >= 0
    b.set_signals_packed(sigs, slot, off)
    return b


def record(engine):
    """{case: [[d2h calls, d2h bytes, device bytes, f32 re-runs] per finish]} on the library the binding has loaded"""
    out = {}
    mdl = models()
    for outlier, table in ((False, SEQUENCES), (True, {k: {"outlier": v} for k, v in OUTLIER.items()})):
        for name, seqs in table.items():
            dm = B.DeviceModel(engine, mdl[name])
            for form in ("rows", "packed"):
                for seq_name, seq in seqs.items():
                    b = _batch(dm, form, outlier)
                    rows = []
                    for flags in seq:
                        _counts()
                        b.run(1.0, flags)
                        b.finish()
                        calls, nbytes = _counts()
                        rows.append([calls, nbytes, b.device_bytes(), b.f32_reruns()])
                    b.close()
                    out["%s,%s,%s" % (name, form, seq_name)] = rows
            dm.close()
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "result_copies.json")
    eng = B.Engine(0)
    table = record(eng)
    eng.close()
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
    print("wrote", out, "from", os.path.dirname(B.__file__), len(table), "cases")


if __name__ == "__main__":
    main()

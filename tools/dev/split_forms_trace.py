#!/usr/bin/env python3
"""Which split-operand layer kernels a fixed set of runs launches, on which grids and how often: the record that holds a change of the host's launch
rules (split_plan, launch_lstm_split, run_front / run_layers / ffhip_batch_run_pair) to the launches of the library before it.

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/dev/split_forms_trace.py run      (FFHIP_BINDING_LIBRARY names the library)
  python tools/dev/split_forms_trace.py compare BEFORE_DIR AFTER_DIR OUT.txt                               (exit 1 when the two multisets differ)

`run` is the recorder of tests/test_split_pair_px_order_gpu.py (pairs, 512- and 768-row launches, ragged and packed, both gate levels), then uniform
one-read-a-row batches of 16, 256, 512, 768 and 1024 rows at every (kind, H) the layer kernels support, each alone and with a second batch between run and
finish, then the projection + recurrence-only path (FFHIP_RUN_UNFUSED_RNN: k_rnn_split) at H = 256 and 512."""
import collections
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NAMES = ("k_lstm_split", "k_lstm_pack", "k_grumod_pack", "k_rnn_split")
ROWS = (16, 256, 512, 768, 1024)
T = 600


def run():
    import numpy as np
    from flappie_amd import binding as B
    from flappie_amd import model as M
    import test_split_pair_px_order_gpu as P

    P.record(B)
    eng = B.Engine(0)
    rng = np.random.default_rng(10)
    shapes = [(M.NET_LSTM5, h) for h in (128, 256, 384, 512)] + [(M.NET_GRUMOD5, h) for h in (128, 256, 384)]
    for kind, hidden in shapes:
        dm = B.DeviceModel(eng, M.synthetic_model(kind, hidden, seed=1))
        other = B.Batch(dm, 256, T)
        other.set_signals(rng.standard_normal((256, T)).astype(np.float32))
        for rows in ROWS:
            b = B.Batch(dm, rows, T)
            b.set_signals(rng.standard_normal((rows, T)).astype(np.float32))
            for beside in (False, True):
                if beside:
                    other.run()
                b.run()
                b.finish()
                assert b.rnn_path() == 3, (kind, hidden, rows, b.rnn_path())
                if beside:
                    other.finish()
            if kind == M.NET_LSTM5 and hidden in (256, 512) and rows in (256, 1024):
                b.run(1.0, B.RUN_UNFUSED_RNN)
                b.finish()
            b.close()
        other.close()
        dm.close()
    eng.close()
    print("split_forms_trace: ran with", os.environ.get("FFHIP_BINDING_LIBRARY") or "the tree's library")


def launches(d):
    """{(kernel name, grid): calls} of the layer kernels in the kernel trace under directory d"""
    out = collections.Counter()
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel trace under " + d
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = r["Kernel_Name"].replace("void ffhip::", "").split("(")[0]
                if any(n in name for n in NAMES):
                    out[(name, "x".join(r[k] for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z")))] += 1
    return out


def compare(before, after, out):
    a, b = launches(before), launches(after)
    lines = []
    for tag, c in (("before", a), ("after", b)):
        lines.append("== %s: %d launches of %d (kernel, grid) kinds   [calls  grid (work items)  kernel]" % (tag, sum(c.values()), len(c)))
        lines += ["%6d  %-12s %s" % (n, k[1], k[0]) for k, n in sorted(c.items())]
    diff = sorted(k for k in set(a) | set(b) if a[k] != b[k])
    lines.append("== comparison: " + ("the two multisets of (kernel, grid, calls) are equal" if not diff else "%d entries differ" % len(diff)))
    lines += ["  before %6d  after %6d  %-12s %s" % (a[k], b[k], k[1], k[0]) for k in diff]
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print(lines[-1 - len(diff)])
    return 1 if diff else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["compare"] and len(sys.argv) == 5:
        sys.exit(compare(*sys.argv[2:5]))
    else:
        sys.exit(__doc__)

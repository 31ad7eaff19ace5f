"""flappie --remap-events on the CPU: the two restatements of include/ffhip.h "events" (events_ref.py) against each other, on random paths and on the inputs that
rule out a one-pass sum of squares; the span arithmetic at its edges; the option and its refusals; the library's new entries.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import events_ref as E
from test_cli import FLAPPIE, ROOT, RUNNIE, needs_hdf5

LIBFFHIP = os.path.join(ROOT, "flappie_amd", "libffhip.so")


def test_the_two_restatements_agree():
    rng = np.random.default_rng(1)
    n = 0
    for stride in (5, 2):
        for N in (1, 2, 63, 64, 65, 257):
            for L in sorted({1, N + 1, int(rng.integers(1, N + 2)), int(rng.integers(1, N + 2))}):
                rm = np.zeros(N, np.uint8)
                rm[rng.choice(N, L - 1, replace=False)] = 1
                for nsample in (N * stride, N * stride - (stride - 1)):
                    x = (rng.standard_normal(nsample) * 3.0 + 1.0).astype(np.float32)
                    a, b = E.events(x, stride, rm, L), E.events_naive(x, stride, rm, L)
                    E.check(a, b, x, (stride, N, L, nsample))
                    assert int(a["count"].sum()) == nsample and np.all(a["count"] >= 0)
                    n += 1
    assert n >= 80
    for name, x, stride, rm, L, constant in E.special_cases():
        a, b = E.events(x, stride, rm, L), E.events_naive(x, stride, rm, L)
        E.check(a, b, x, name)
        if constant:
            for ev in (a, b):
                assert np.array_equal(ev["mean"], x[ev["first"]]) and np.all(ev["sd"] == 0.0), (name, ev)


def test_span_arithmetic_and_its_edges():
    # four bases over seven blocks of stride 5: starts 0, 3, 5, 6
    rm = np.array([0, 0, 1, 0, 1, 1, 0], np.uint8)
    s, c = E.spans(35, 5, rm, 4)
    assert s.tolist() == [0, 15, 25, 30] and c.tolist() == [15, 10, 5, 5]
    assert np.array_equal(E.rm_of_starts([0, 3, 5, 6], 7), rm)
    # n < N stride: the chain of ceilings rounded up, the last block is short -- or, two blocks short, wholly beyond the signal
    s, c = E.spans(31, 5, rm, 4)
    assert s.tolist() == [0, 15, 25, 30] and c.tolist() == [15, 10, 5, 1]
    s, c = E.spans(27, 5, rm, 4)
    assert s.tolist() == [0, 15, 25, 27] and c.tolist() == [15, 10, 2, 0]
    # L = N + 1: every base one block, the last none
    s, c = E.spans(15, 5, np.ones(3, np.uint8), 4)
    assert s.tolist() == [0, 5, 10, 15] and c.tolist() == [5, 5, 5, 0]
    ev = E.events(np.arange(15, dtype=np.float32), 5, np.ones(3, np.uint8), 4)
    assert ev["mean"].tolist() == [2.0, 7.0, 12.0, 0.0] and ev["sd"][3] == 0.0 and abs(float(ev["sd"][0]) - 2.0 ** 0.5) < 1e-7
    # L = 1: one base owns everything
    s, c = E.spans(33, 5, np.zeros(7, np.uint8), 1)
    assert s.tolist() == [0] and c.tolist() == [33]
    assert E.EVENT_DTYPE.itemsize == 16
    assert [E.rm_of_lengths(k).tolist() for k in ([2, 1], [1, 1, 0])] == [[0, 1, 0], [1, 1]]


@needs_hdf5
def test_option_and_its_refusals_without_gpu(tmp_path):
    refs = tmp_path / "refs.fa"
    refs.write_text(">r1\nACGT\n")
    r = subprocess.run([FLAPPIE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--remap-events=" in r.stdout
    for line in r.stdout.split("\n"):                           # a long option only
        if "--remap-events=" in line:
            assert re.match(r"^ {6}--remap-events=", line), line
    r = subprocess.run([RUNNIE, "--help"], capture_output=True, text=True, timeout=60)
    assert "--remap-events" not in r.stdout

    def refused(exe, *args):
        r = subprocess.run([exe] + list(args) + [str(tmp_path / "none.fast5")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and r.stdout == "", args
        return r.stderr
    out = tmp_path / "events.tsv"
    assert "--remap-events goes with --remap" in refused(FLAPPIE, "--remap-events", str(out))
    assert "--remap-events" in refused(RUNNIE, "--remap-events", str(out))
    assert "--remap-out" in refused(FLAPPIE, "--remap", str(refs), "--remap-events", str(out))
    assert not out.exists()


def test_library_exports_the_new_entries():
    lib = C.CDLL(LIBFFHIP)
    for name in ("ffhip_batch_events", "ffhip_op_events"):
        assert hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "ffhip.h")).read()
    assert re.search(r"#define\s+FFHIP_RUN_EVENTS\s+131072u", text)
    from flappie_amd import binding
    assert binding.RUN_EVENTS == 131072 and hasattr(binding.Batch, "events") and hasattr(binding, "op_events") and binding.EVENT_DTYPE == E.EVENT_DTYPE

#!/usr/bin/env python3
"""tests/golden/annot_copies.json: what every finished run of the cases below copies to the host, what its batch holds on the device and what its per-read
products OUTSIDE the result block are (barcodes, adapters, truth, remap, events, site mods, variants), recorded from the release library of the commit BEFORE
those products were described by a table (flappie_amd/csrc/ffhip_annot.hpp).  tests/test_annot_copies_gpu.py runs the same cases (record() below) on the
library of its tree and holds it to these figures exactly.

This script runs in a built checkout of that parent (copied to its tests/golden/: it imports the flappie_amd beside it, whose binding matches that library)
and needs a GPU:
usage: PARENT/tests/golden/make_annot_copies.py [OUT.json]
It runs every case twice and writes nothing if a figure or a digest differs between the two.

Per case, after each finish of its flag sequence: [device-to-host copy calls, device-to-host bytes (ffhip_copy_counts, reset before the run), device bytes the
batch holds (ffhip_debug_batch_device_bytes), reads run again on the f32 path, {feature: SHA-256 of its records over all reads, as the binding returns them}]."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_result_copies as G  # noqa: E402
import variants_ref as V  # noqa: E402
from test_variants_gpu import _variants  # noqa: E402

B = G.B
# launch order; (flag, accessor); the last three go with RUN_REMAP
FEATURES = {"barcodes": (B.RUN_BARCODES, "barcode"), "adapters": (B.RUN_ADAPTERS, "adapters"), "truth": (B.RUN_TRUTH, "truth"), "remap": (B.RUN_REMAP, "remap"),
            "events": (B.RUN_EVENTS, "events"), "site_mods": (B.RUN_REMAP_MODS, "site_mods"), "variants": (B.RUN_REMAP_VARIANTS, "variant_calls")}
WITH_REMAP = ("events", "site_mods", "variants")
ALL = 0
for _f, _ in FEATURES.values():
    ALL |= _f
BARCODES = ("ACGTACCGTTAGCATGGACTTCAG", "TTGACCATGCAAGTCCGATAGGCA")
ADAPTERS = ("AATGTACTTCGTTCAGTTACGTATTGCT", "GCAATACGTAACTGAACGAAGT")
NBASE = 5


def alone(name):
    return FEATURES[name][0] | (B.RUN_REMAP if name in WITH_REMAP else 0)


# flag sequences: each feature created, absent, there again; all seven; all seven, the inputs twice as long ("double": applied in front of that run), all seven
SEQUENCES = {name: (alone(name), 0, alone(name)) for name in FEATURES}
SEQUENCES["all"] = (ALL,)
SEQUENCES["grow"] = (ALL, "double", ALL)
FORMS = (("rows", False), ("rows", True), ("packed", False), ("packed", True))      # (batch form, outlier in read 1)


def _blob(x):
    """a record of the binding as bytes: dicts by key, arrays and numpy scalars by their bytes"""
    if x is None:
        return b"-"
    if isinstance(x, dict):
        return b"{" + b",".join(k.encode() + b":" + _blob(x[k]) for k in sorted(x)) + b"}"
    if isinstance(x, (list, tuple)):
        return b"[" + b",".join(_blob(v) for v in x) + b"]"
    if isinstance(x, (np.ndarray, np.generic)):
        return str(x.dtype).encode() + b"(" + np.ascontiguousarray(x).tobytes() + b")"
    return repr(x).encode()


def _inputs(b, times):
    """the reads' own calls (`times` times over) as remap sequences and truths, and their variants"""
    seqs = []
    for v in range(b.nreads()):
        call = b.basecall(v)
        seqs.append(np.array([("ACGTZ".index(x)) for x in call] * times, np.uint8) if call else np.array([1] * times, np.uint8))
    b.set_remap(seqs, 2048)
    b.set_truth(seqs, 512)
    b.set_remap_variants([V.pack(_variants(np.random.default_rng(1000 + v), q, NBASE, 3)) for v, q in enumerate(seqs)], 10, False)


def record(engine, blobs=None):
    """{case: [[d2h calls, d2h bytes, device bytes, f32 re-runs, {feature: digest}] per finish]} on the library the binding has loaded.
    blobs: a dict that receives {(case, finish, feature): [every read's record as bytes]}"""
    out = {}
    dm = B.DeviceModel(engine, G.models()["lstm5mod"])
    bc, ad = B.Barcodes(engine, BARCODES), B.Adapters(engine, ADAPTERS)
    for form, outlier in FORMS:
        for seq_name, seq in SEQUENCES.items():
            case = "%s,%s,%s" % (form, "outlier" if outlier else "clean", seq_name)
            b = G._batch(dm, form, outlier)
            b.run(1.0, 0)
            b.finish()
            b.set_barcodes(bc)
            b.set_adapters(ad)
            _inputs(b, 1)
            rows = []
            for flags in seq:
                if flags == "double":
                    _inputs(b, 2)
                    continue
                G._counts()
                b.run(1.0, flags)
                b.finish()
                calls, nbytes = G._counts()
                digests = {}
                for name, (flag, getter) in FEATURES.items():
                    if flags & flag:
                        recs = [_blob(getattr(b, getter)(v)) for v in range(b.nreads())]
                        digests[name] = hashlib.sha256(b"|".join(recs)).hexdigest()
                        if blobs is not None:
                            blobs[(case, len(rows), name)] = recs
                rows.append([calls, nbytes, b.device_bytes(), b.f32_reruns(), digests])
            b.close()
            out[case] = rows
    bc.close()
    ad.close()
    dm.close()
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "annot_copies.json")
    eng = B.Engine(0)
    table, again = record(eng), record(eng)
    eng.close()
    bad = [k for k in table if table[k] != again[k]]
    if bad:
        for k in bad:
            print("NOT REPRODUCIBLE", k, table[k], again[k])
        sys.exit(1)
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join('"%s":%s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in table.items()) + "\n}\n")
    print("wrote", out, "from", os.path.dirname(B.__file__), len(table), "cases")


if __name__ == "__main__":
    main()

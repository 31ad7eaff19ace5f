"""Multi-read fast5 files (one file, a root group read_<x> per read) through the cursor of include/fast5_interface.h: fast5_multi_open / _next / _close.
As for single-read files there are two paths -- host/fast5_raw.c's walker over the mapped file, and libhdf5 for whatever the walker refuses -- and they must
give the same reads in the same order: increasing strcmp order of the group names, each read as the file holds it (int16 DAC values, read id, offset and
raw_unit = range / digitisation in float).  The files are written by `fast5_tool writem` in every layout it knows; none is committed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from test_fast5_raw import FAST5LIB, TOOL, RawTable, needs_hdf5, writex

F = np.float32
# writem's flags: 1 chunked, 2 deflate, 4 shuffle, 32 latest format (dense links in a root group of nine), 1024 no file_type, 2048 no read_id, 4096 unsorted creation order
CHUNKED, DEFLATE, SHUFFLE, LATEST, NO_FILE_TYPE, NO_READ_ID, UNSORTED = 1, 2, 4, 32, 1024, 2048, 4096
LAYOUTS = [(0, 0), (CHUNKED, 1000), (CHUNKED | DEFLATE, 512), (CHUNKED | DEFLATE | SHUFFLE, 1000), (NO_FILE_TYPE, 0), (NO_READ_ID, 0), (UNSORTED, 0),
           (UNSORTED | CHUNKED | DEFLATE | SHUFFLE | NO_FILE_TYPE | NO_READ_ID, 300), (LATEST, 0), (LATEST | CHUNKED | DEFLATE | SHUFFLE | UNSORTED, 1000)]


class DacRead(C.Structure):
    _fields_ = [("uuid", C.c_void_p), ("dac", C.POINTER(C.c_int16)), ("n", C.c_size_t), ("offset", C.c_float), ("raw_unit", C.c_float)]


def load():
    L = C.CDLL(FAST5LIB)
    L.fast5_multi_open.restype = C.c_void_p
    L.fast5_multi_open.argtypes = [C.c_char_p]
    L.fast5_multi_open_path.restype = C.c_void_p
    L.fast5_multi_open_path.argtypes = [C.c_char_p, C.c_int]
    L.fast5_multi_next.argtypes = [C.c_void_p, C.POINTER(DacRead)]
    L.fast5_multi_close.argtypes = [C.c_void_p]
    L.fast5_multi_count.restype = C.c_size_t
    L.fast5_multi_count.argtypes = [C.c_void_p]
    L.read_raw.restype = RawTable
    L.read_raw.argtypes = [C.c_char_p, C.c_bool]
    return L


@pytest.fixture(scope="module")
def lib():
    return load()


def walk(L, path, which=0):
    """every read the cursor gives: None if the file is refused, else a list of (uuid, samples, offset, raw_unit) -- or None for a read that was skipped"""
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    m = L.fast5_multi_open_path(str(path).encode(), which)
    if not m:
        return None
    out = []
    assert L.fast5_multi_count(m) < 1 << 20
    while True:
        r = DacRead()
        rc = L.fast5_multi_next(m, C.byref(r))
        if rc == 0:
            break
        if rc < 0:
            assert not r.dac and not r.uuid
            out.append(None)
            continue
        out.append((C.string_at(r.uuid).decode("latin-1"), np.ctypeslib.as_array(r.dac, shape=(r.n,)).copy(), r.offset, r.raw_unit))
        libc.free(r.uuid)
        libc.free(C.cast(r.dac, C.c_void_p))
    L.fast5_multi_close(m)
    return out


def make_reads():
    """nine reads: lengths 1, 2, 3, 5, 100, 4097 and three between 1000 and 9000; group names that are not in the list's order; a calibration each"""
    rng = np.random.default_rng(7)
    lens = [1, 2, 3, 5, 100, 4097, 1000, 4000, 8999]
    names = ["7f3a", "00c1", "zz09", "a1b2", "Z_up", "3e3e", "a1b20", "0fff", "b000"]
    reads = []
    for k, (n, name) in enumerate(zip(lens, names)):
        reads.append(dict(name=name, id="id-%d-%s" % (k, name), dac=rng.integers(-2000, 9000, n).astype(np.int16),
                          dig=[8192.0, 2048.0, 8192.0][k % 3], off=[16.0, -231.0, 3.4375][k % 3], rng=1373.41 + 7.25 * k))
    return reads


def writem(path, reads, flags=0, chunk=0, filtered=()):
    lines = []
    for k, r in enumerate(reads):
        sf = "%s.%d.i16" % (path, k)
        np.asarray(r["dac"], dtype="<i2").tofile(sf)
        lines.append("%s %s %r %r %r %s%s" % (r["name"], r["id"], r["dig"], r["off"], r["rng"], sf, " filter" if k in filtered else ""))
    lst = str(path) + ".list"
    with open(lst, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    subprocess.run([TOOL, "writem", str(path), str(flags), str(chunk), lst], check=True)


def expected(reads, flags):
    out = []
    for r in sorted(reads, key=lambda r: ("read_" + r["name"]).encode()):
        out.append((r["name"] if flags & NO_READ_ID else r["id"], r["dac"], F(r["off"]), F(r["rng"]) / F(r["dig"])))
    return out


def same(got, want):
    assert got is not None and len(got) == len(want)
    for g, w in zip(got, want):
        assert g is not None and g[0] == w[0]
        assert g[1].dtype == np.int16 and np.array_equal(g[1], w[1])
        assert F(g[2]) == w[2] and F(g[3]) == w[3], (g[2:], w[2:])


@needs_hdf5
@pytest.mark.parametrize("flags,chunk", LAYOUTS)
def test_cursor_on_every_layout(tmp_path, lib, flags, chunk):
    reads = make_reads()
    p = tmp_path / "multi.fast5"
    writem(p, reads, flags, chunk)
    want = expected(reads, flags)
    assert [w[0] for w in want] != [(r["name"] if flags & NO_READ_ID else r["id"]) for r in reads], "the fixture's list is in name order: the order is not tested"
    through_hdf5 = walk(lib, p, 2)
    same(through_hdf5, want)
    walker = walk(lib, p, 1)
    if flags & LATEST:
        assert walker is None, "the walker read a root group with dense link storage: this case no longer tests the fallback"
    else:
        same(walker, want)                        # ... so the two paths agree value for value
    same(walk(lib, p, 0), want)                   # the cursor as the binaries use it delivers either way
    # a multi-read file is no single-read file, and the other way round
    assert not lib.read_raw(str(p).encode(), True).raw


@needs_hdf5
def test_single_read_files_scale_as_the_device_does(tmp_path, lib):
    """the same nine reads as single-read files: read_raw's floats are (dac + offset) * raw_unit in float32, the expression k_dac_to_pa evaluates
    (tests/test_prep_dac_gpu.py holds the kernel to the same numpy line) -- and no single-read file is taken for a multi-read one"""
    for k, r in enumerate(make_reads()):
        p = tmp_path / ("single_%d.fast5" % k)
        writex(p, r["id"], r["dac"], 0, dig=r["dig"], off=r["off"], rng=r["rng"])
        rt = lib.read_raw(str(p).encode(), True)
        assert rt.raw and rt.n == r["dac"].size and rt.uuid == r["id"].encode()
        got = np.ctypeslib.as_array(rt.raw, shape=(rt.n,)).copy()
        want = ((r["dac"].astype(F) + F(r["off"])) * (F(r["rng"]) / F(r["dig"]))).astype(F)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        for which in (0, 1, 2):
            assert walk(lib, p, which) is None


# ---- files that are wrong: run in a child process, so that a crash of the reader is a failed assertion and its messages can be read ---------------
CHILD = r"""
import sys
sys.path.insert(0, %(tests)r)
import numpy as np
import test_fast5_multi as T
L = T.load()
%(body)s
"""


def child(body, env=None):
    code = CHILD % dict(tests=os.path.dirname(os.path.abspath(__file__)), body=body)
    e = dict(os.environ)
    e.pop("HDF5_PLUGIN_PATH", None)
    e.update(env or {})
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=120)


@needs_hdf5
def test_object_header_size_that_wraps(tmp_path):
    """a version-2 object header whose chunk-0 size field is eight bytes of 0xff: size + 4 wraps to 3, the bounds check passed, and the parser was
    handed 2^64 bytes.  Both readers (they are one parser) must refuse the file."""
    reads = make_reads()[:3]
    single, multi = tmp_path / "s.fast5", tmp_path / "m.fast5"
    writex(single, "wrap", reads[2]["dac"], 32)
    writem(multi, reads, LATEST)
    for p in (single, multi):
        d = bytearray(p.read_bytes())
        pos, hits = d.find(b"OHDR"), 0
        while pos >= 0:
            fl = d[pos + 5]
            off = pos + 6 + (16 if fl & 0x20 else 0) + (4 if fl & 0x10 else 0)
            d[pos + 5] = fl | 3                       # the size field is 8 bytes wide ...
            d[off:off + 8] = b"\xff" * 8              # ... and holds 2^64 - 1
            hits += 1
            pos = d.find(b"OHDR", pos + 4)
        assert hits > 0
        p.write_bytes(bytes(d))
    # ... and with nothing but zeros behind the first such header (they parse as empty messages, one after the other): a parser that believed the size
    # walks off the end of the mapped file
    d = bytearray(multi.read_bytes())
    pos = d.find(b"OHDR")
    off = pos + 6 + (16 if d[pos + 5] & 0x20 else 0) + (4 if d[pos + 5] & 0x10 else 0) + 8
    d[off:] = bytes(len(d) - off)
    zeros = tmp_path / "z.fast5"
    zeros.write_bytes(bytes(d))
    r = child("""
fr = T.C.create_string_buffer(64)
L.fast5_read_raw_fast.argtypes = [T.C.c_char_p, T.C.c_int, T.C.c_void_p]
assert L.fast5_read_raw_fast(%r, 1, fr) == 0
assert T.walk(L, %r, 1) is None
assert T.walk(L, %r, 1) is None
print("refused")
""" % (str(single).encode(), str(multi), str(zeros)))
    assert r.returncode == 0 and "refused" in r.stdout, (r.returncode, r.stderr[-2000:])


@needs_hdf5
def test_chunk_listed_twice(tmp_path):
    """a chunk B-tree that lists one chunk twice and another not at all still 'covers' every element by count; the samples of the missing chunk were
    never written.  The walker must refuse such a Signal (or give the true samples), never return what malloc left"""
    r0 = dict(make_reads()[7])
    r0["dac"] = np.arange(1, 2001, dtype=np.int16)
    p = tmp_path / "dup.fast5"
    writem(p, [r0], CHUNKED, 500)
    d = bytearray(p.read_bytes())
    pos = d.find(b"TREE")
    while pos >= 0 and d[pos + 4] != 1:
        pos = d.find(b"TREE", pos + 4)
    assert pos >= 0 and d[pos + 5] == 0 and int.from_bytes(d[pos + 6:pos + 8], "little") == 4, "one leaf with the four chunks was expected"
    ent = lambda i: pos + 24 + i * 32                  # key {size, mask, offset[2]} = 24 bytes, child address = 8
    assert int.from_bytes(d[ent(2) + 8:ent(2) + 16], "little") == 1000
    d[ent(2):ent(2) + 32] = d[ent(1):ent(1) + 32]      # the chunk at 500 twice, the one at 1000 never
    p.write_bytes(bytes(d))
    r = child("""
for rep in range(8):
    junk = [np.full(1000, 0x5555, dtype=np.int16) for _ in range(4)]      # what a recycled allocation would hold
    del junk
    got = T.walk(L, %r, 1)
    assert got is not None and len(got) == 1
    assert got[0] is None or np.array_equal(got[0][1], np.arange(1, 2001, dtype=np.int16)), got[0][1][990:1010]
print("held")
""" % str(p))
    assert r.returncode == 0 and "held" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


@needs_hdf5
def test_byte_flips_never_crash_the_walker(tmp_path):
    """300 files with three bytes changed each (structures and data alike): the cursor over the walker returns reads or refuses -- it reads nothing
    outside the mapped file (every access behind one bounds check)"""
    p = tmp_path / "flip.fast5"
    writem(p, make_reads(), CHUNKED | DEFLATE | SHUFFLE, 700)
    r = child("""
data = open(%r, "rb").read()
rng = np.random.default_rng(2)
refused = delivered = 0
for k in range(300):
    d = bytearray(data)
    span = len(d) if k %% 3 == 0 else min(len(d), 8192)
    for pos in rng.integers(0, span, size=3):
        d[pos] = int(rng.integers(0, 256))
    open(%r, "wb").write(bytes(d))
    got = T.walk(L, %r, 1)
    if got is None:
        refused += 1
    else:
        refused += sum(g is None for g in got)
        delivered += sum(g is not None for g in got)
print("refused", refused, "delivered", delivered)
assert refused > 0 and delivered > 0
""" % (str(p), str(tmp_path / "bad.fast5"), str(tmp_path / "bad.fast5")))
    assert r.returncode == 0 and "refused" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


@needs_hdf5
def test_filter_without_plugin_skips_one_read(tmp_path):
    """one read's Signal names HDF5 filter 32020 (VBZ) and no plugin is to be found: that read is skipped with a message that names the filter, the
    others are delivered, in order"""
    reads = make_reads()
    p = tmp_path / "vbz.fast5"
    writem(p, reads, 0, 256, filtered=(7,))
    r = child("""
got = T.walk(L, %r, 0)
want = T.expected(T.make_reads(), 0)
skipped = [i for i, g in enumerate(got) if g is None]
assert len(got) == len(want) and skipped == [[w[0] for w in want].index("id-7-0fff")], skipped
T.same([g for g in got if g is not None], [w for i, w in enumerate(want) if i not in skipped])
print("skipped", skipped)
""" % str(p))
    assert r.returncode == 0 and "skipped" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert "32020" in r.stderr and "id-7-0fff" in r.stderr

"""The library's exclusive prefix sums (csrc/am_scan.hip: launch_scan, launch_scan64, launch_scan_jobs, launch_offsets_rebase) as a test sees them: the sizes and
the inputs at which a sum can slip, the definition, and the calls into libam_scancheck.so (tests/native/am_scan_check.hip -- am_scan.hip itself, compiled with the
product's flags, behind a C interface).  Shared by tests/test_scan_cases_cpu.py (the definition against Python integers, the size lists against the seams, the
build) and tests/test_gpu_scan_sums.py (the kernels).

The definition: out[i] = (in[0] + ... + in[i - 1]) mod 2^64 -- numpy's cumsum on uint64, shifted by one.

The seams come from the library (amsc_limits), never from a literal: a tile of T elements is summed by one workgroup whose lanes hold P = T / sweep elements each,
W = 64 P per wavefront; ONE workgroup then sums the tile sums in sweeps of `sweep` tiles with a carry, so S = sweep x T elements is the first size whose last
tile gets its base through the carry.  k_scan_jobs gives a lane 4 elements, a wavefront 256, a sweep T, and issues the loads of four sweeps together."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

from alfred_margaret_amd import build

WAVE = 64
FILL = 0xA5A5A5A5A5A5A5A5                                  # what the guard behind `out` (and all of `out` before a call) holds
MAX_CASE_BYTES = 64 << 20
INVALID_VALUE = 1                                          # hipErrorInvalidValue
U32_MAX, U64_TOP = 0xFFFFFFFF, 1 << 63
SPIKE = {4: 0xFFFFFFFF, 8: 0xFEDCBA9876543210}
JOB_LANE, JOB_WAVE = 4, 256                                # elements per lane and per wavefront of k_scan_jobs

Limits = namedtuple("Limits", "tile tiles_sweep spans_tile spans_threads spans_tiles_sweep near_lds_needles max_jobs")


class Job(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("n", C.c_uint64), ("n_dev_value", C.c_uint64), ("kind", C.c_uint32), ("has_n_dev", C.c_uint32)]


_lib = None


def lib():
    """libam_scancheck.so, built on demand; nothing but the tests loads it."""
    global _lib
    if _lib is None:
        path = os.path.join(build.LIB, "libam_scancheck.so")
        if not os.path.exists(path):
            path = build.build_scancheck()
        x = C.CDLL(path)
        x.amsc_guard_items.restype = C.c_uint64
        x.amsc_limits.argtypes = [C.POINTER(C.c_uint64)]
        x.amsc_limits.restype = None
        x.amsc_scan_temp_bytes.argtypes, x.amsc_scan_temp_bytes.restype = [C.c_uint64], C.c_uint64
        for f in (x.amsc_scan32, x.amsc_scan64):
            f.argtypes, f.restype = [C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p], C.c_int
        x.amsc_scan_jobs.argtypes, x.amsc_scan_jobs.restype = [C.POINTER(Job), C.c_uint32], C.c_int
        x.amsc_offsets_rebase.argtypes, x.amsc_offsets_rebase.restype = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p], C.c_int
        _lib = x
    return _lib


def limits():
    out = (C.c_uint64 * 7)()
    lib().amsc_limits(out)
    return Limits(*[int(v) for v in out])


def guard():
    return int(lib().amsc_guard_items())


# ---- the sizes

def seams(lim):
    """(P, W, T, S): elements of a lane, a wavefront, a tile, and of the first sweep of the pass over the tile sums."""
    t = lim.tile
    p = t // lim.tiles_sweep
    return p, WAVE * p, t, lim.tiles_sweep * t


def scan_sizes(lim):
    p, w, t, s = seams(lim)
    return [1, 2, p - 1, p, p + 1, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t + 1, s - 1, s, s + 1, s + t + 1, 2 * s + w + 1]


def job_seams(lim):
    return JOB_LANE, JOB_WAVE, lim.tile, 4 * lim.tile


def job_sizes(lim):
    t = lim.tile
    return [0, 1, 3, 4, 5, 255, 256, 257, t - 1, t, t + 1, 4 * t - 1, 4 * t, 4 * t + 1, 8 * t + 5, 1 << 16, 1 << 18]


def n_dev_pairs(lim):
    """(*n_dev, j.n) of the device-side length of k_scan_jobs"""
    t = lim.tile
    return [(0, 0), (0, 1), (t - 1, 1), (t, 1), (4 * t, 1), (5, 4 * t)]


def spike_positions(lim, n, jobs=False):
    p, w, t, s = seams(lim)
    at = {0, p - 1, p, w - 1, w, t - 1, t, s - 1, s, n - 1}
    if jobs:
        at |= {JOB_LANE - 1, JOB_LANE, JOB_WAVE - 1, JOB_WAVE, 4 * t - 1, 4 * t}
    return sorted(x for x in at if 0 <= x < n)


def case_bytes(n, width):
    """host bytes of one case: the input, the output with its guard, the expected output"""
    return n * width + 2 * (n + guard()) * 8


# ---- the inputs

def dtype_of(width):
    return np.uint32 if width == 4 else np.uint64


def patterns(lim, width, n, jobs=False):
    """(name, input) for every pattern of the size: ones (the answer is the index), all 0xFFFFFFFF (a uint32 sum crosses 2^32 at the second element of every lane),
    random values of the full 32-bit range, one spike per seam position; 64-bit inputs also wrap: random 64-bit values, all 2^63."""
    dt = dtype_of(width)
    rng = np.random.default_rng(1000003 * width + n)
    yield "ones", np.ones(n, dt)
    yield "all 0xFFFFFFFF", np.full(n, U32_MAX, dt)
    yield "random", rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(dt)
    for at in spike_positions(lim, n, jobs):
        x = np.zeros(n, dt)
        x[at] = SPIKE[width]
        yield "spike at %d" % at, x
    if width == 8:
        yield "random 64-bit", rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False) if n else np.zeros(0, np.uint64)
        yield "all 2^63", np.full(n, U64_TOP, np.uint64)


def reference(x):
    """out[i] = (x[0] + ... + x[i - 1]) mod 2^64"""
    out = np.zeros(len(x), np.uint64)
    if len(x) > 1:
        np.cumsum(x[:-1].astype(np.uint64), dtype=np.uint64, out=out[1:])
    return out


def reference_python(x):
    """the same in Python integers"""
    out, run = [], 0
    for v in x:
        out.append(run)
        run = (run + int(v)) % (1 << 64)
    return out


# ---- the calls: every one returns (launcher's error, out with its guard)

def fresh_out(n):
    return np.full(n + guard(), FILL, np.uint64)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def scan(x, temp_bytes=-1):
    x = np.ascontiguousarray(x)
    out = fresh_out(len(x))
    f = lib().amsc_scan32 if x.dtype == np.uint32 else lib().amsc_scan64
    assert x.dtype in (np.uint32, np.uint64)
    return f(_ptr(x), len(x), temp_bytes, _ptr(out)), out


def scan_temp_bytes(n):
    return int(lib().amsc_scan_temp_bytes(n))


def scan_jobs(jobs):
    """jobs: (input, n_dev) -- n_dev None: the length is the host's; otherwise the first n_dev elements are announced by the device word, the rest by j.n"""
    arr = (Job * max(len(jobs), 1))()
    keep, outs = [], []
    for k, (x, n_dev) in enumerate(jobs):
        x = np.ascontiguousarray(x)
        assert x.dtype in (np.uint32, np.uint64) and (n_dev is None or n_dev <= len(x))
        out = fresh_out(len(x))
        keep.append(x)
        outs.append(out)
        arr[k] = Job(x.ctypes.data, out.ctypes.data, len(x) - (n_dev or 0), n_dev or 0, 0 if x.dtype == np.uint32 else 1, 0 if n_dev is None else 1)
    return lib().amsc_scan_jobs(arr, len(jobs)), outs


def offsets_rebase(local, n, base):
    out = fresh_out(n)
    if local is not None:
        local = np.ascontiguousarray(local, np.uint64)
        assert len(local) == n
    return lib().amsc_offsets_rebase(None if local is None else _ptr(local), n, base, _ptr(out)), out


def mismatch(out, x, what):
    """None when `out` is the exclusive sum of x followed by an untouched guard; otherwise a short description"""
    n = len(x)
    if len(out) != n + guard():
        return "%s: %d elements came back, %d expected" % (what, len(out), n + guard())
    if not (out[n:] == np.uint64(FILL)).all():
        return "%s: the guard behind out[%d] was written" % (what, n)
    exp = reference(x)
    bad = np.flatnonzero(out[:n] != exp)
    if len(bad):
        i = int(bad[0])
        return "%s: out[%d] = %d, expected %d (%d of %d differ)" % (what, i, int(out[i]), int(exp[i]), len(bad), n)
    return None

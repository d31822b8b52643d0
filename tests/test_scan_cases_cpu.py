"""(CPU) What tests/test_gpu_scan_sums.py rests on (tests/scan_cases.py): the definition of the exclusive sum against Python integers, the size lists against the
seams the library reports, the cost of a case, and the test library itself -- it cross-compiles for gfx950 and exports its C interface and nothing else."""
import subprocess

import numpy as np

import alfred_margaret_amd as am
from tests import scan_cases as sc


def test_scancheck_builds_and_exports_its_interface():
    path = am.build.build_scancheck()
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    got = sorted(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert got == ["amsc_guard_items", "amsc_limits", "amsc_offsets_rebase", "amsc_scan32", "amsc_scan64", "amsc_scan_jobs", "amsc_scan_temp_bytes"]


def test_limits_are_the_librarys():
    lim = sc.limits()
    assert lim.tile == am.api.select_geometry()[1]                       # scan_tile_items(), through the product's own ABI
    assert lim.tile % lim.tiles_sweep == 0 and lim.spans_tile % lim.spans_threads == 0 and lim.max_jobs == 6
    assert sc.guard() == 64
    p, w, t, s = sc.seams(lim)
    assert 2 < p < w < t < s and 4 * t > sc.JOB_WAVE + 1


def test_the_definition_against_python_integers():
    rng = np.random.default_rng(5)
    cases = [np.zeros(0, np.uint32), np.array([7], np.uint32), np.full(9, sc.U32_MAX, np.uint32), rng.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32),
             np.zeros(0, np.uint64), np.array([sc.U64_TOP], np.uint64), np.full(7, sc.U64_TOP, np.uint64), np.full(5, (1 << 64) - 1, np.uint64),
             rng.integers(0, 1 << 64, 300, dtype=np.uint64, endpoint=False)]
    wrapped = 0
    for x in cases:
        got = sc.reference(x)
        assert got.dtype == np.uint64 and got.tolist() == sc.reference_python(x.tolist())
        wrapped += sum(int(v) for v in x.tolist()) >= 1 << 64
    assert wrapped == 3                                                  # the three 64-bit arrays of more than one large element
    assert sc.reference(np.full(4, sc.U32_MAX, np.uint32)).tolist() == [0, 0xFFFFFFFF, 0x1FFFFFFFE, 0x2FFFFFFFD]      # a uint32 input is widened before it is added
    assert sc.reference(np.full(4, sc.U64_TOP, np.uint64)).tolist() == [0, 1 << 63, 0, 1 << 63]


def test_size_lists_hold_every_seam_with_both_neighbours():
    lim = sc.limits()
    sizes = sc.scan_sizes(lim)
    for seam in sc.seams(lim):
        assert {seam - 1, seam, seam + 1} <= set(sizes), seam
    p, w, t, s = sc.seams(lim)
    assert max(sizes) == 2 * s + w + 1 and s + t + 1 in sizes and min(sizes) == 1 and len(set(sizes)) == len(sizes)
    jobs = sc.job_sizes(lim)
    for seam in sc.job_seams(lim):
        assert {seam - 1, seam, seam + 1} <= set(jobs), seam
    assert 0 in jobs and 8 * t + 5 in jobs and len(set(jobs)) == len(jobs)
    for n_dev, n in sc.n_dev_pairs(lim):
        assert n_dev + n <= 4 * t + 5
    assert {(0, 0), (t, 1), (4 * t, 1)} <= set(sc.n_dev_pairs(lim))


def test_no_case_exceeds_its_budget():
    lim = sc.limits()
    for width in (4, 8):
        for n in sc.scan_sizes(lim) + sc.job_sizes(lim):
            assert sc.case_bytes(n, width) <= sc.MAX_CASE_BYTES, (width, n)
    assert sc.case_bytes(max(sc.scan_sizes(lim)), 8) > 16 << 20         # ... and the largest one is beyond the second sweep


def test_patterns_and_spikes():
    lim = sc.limits()
    p, w, t, s = sc.seams(lim)
    assert sc.spike_positions(lim, 1) == [0] and sc.spike_positions(lim, p) == [0, p - 1]
    assert sc.spike_positions(lim, s + 1) == [0, p - 1, p, w - 1, w, t - 1, t, s - 1, s]
    assert sc.spike_positions(lim, 2 * s) == [0, p - 1, p, w - 1, w, t - 1, t, s - 1, s, 2 * s - 1]
    assert {3, 4, 255, 256, 4 * t - 1, 4 * t} <= set(sc.spike_positions(lim, 4 * t + 1, jobs=True))
    for width in (4, 8):
        for n in (0, 1, t + 1):
            got = list(sc.patterns(lim, width, n))
            names = [k for k, _ in got]
            assert names[:3] == ["ones", "all 0xFFFFFFFF", "random"] and len(set(names)) == len(names)
            assert ("all 2^63" in names) == (width == 8) and ("random 64-bit" in names) == (width == 8)
            assert sum(k.startswith("spike") for k in names) == len(sc.spike_positions(lim, n))
            for k, x in got:
                assert x.dtype == sc.dtype_of(width) and len(x) == n, k
                if k.startswith("spike"):
                    assert np.count_nonzero(x) == 1 and int(x.max()) == sc.SPIKE[width]
    x32 = dict(sc.patterns(lim, 4, t + 1))
    assert int(sc.reference(x32["all 0xFFFFFFFF"])[2]) > 1 << 32 and int(x32["random"].max()) > 1 << 31
    x64 = dict(sc.patterns(lim, 8, t + 1))
    assert int(x64["random 64-bit"].max()) > 1 << 63


def test_mismatch_sees_what_it_is_for():
    x = np.arange(10, dtype=np.uint32)
    good = np.concatenate([sc.reference(x), np.full(sc.guard(), sc.FILL, np.uint64)])
    assert sc.mismatch(good, x, "ok") is None
    for at, word in ((3, "out[3]"), (10, "guard"), (10 + sc.guard() - 1, "guard")):
        bad = good.copy()
        bad[at] += np.uint64(1)
        assert word in sc.mismatch(bad, x, "bad")
    assert "elements" in sc.mismatch(good[:-1], x, "short")

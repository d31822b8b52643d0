"""The library's exclusive prefix sums on the device (csrc/am_scan.hip) against the definition, out[i] = (in[0] + ... + in[i - 1]) mod 2^64 = numpy's cumsum on
uint64 (tests/scan_cases.py; held to Python integers by tests/test_scan_cases_cpu.py).  The launchers are called directly, through libam_scancheck.so
(tests/native/am_scan_check.hip: am_scan.hip itself with the product's flags), on inputs the stages that use them never produce: sums that cross 2^32 and 2^64
inside a lane, a wavefront and a tile, one spike on either side of every seam, and sizes beyond the first sweep of the one-workgroup pass over the tile sums.
Every call hands back `out` with a guard behind it: nothing beyond n is written, and with n == 0 nothing at all."""
import numpy as np
import pytest

from tests import scan_cases as sc

pytestmark = pytest.mark.gpu

LIM = sc.limits()
WIDTHS = {"u32": 4, "u64": 8}


def failures(width, n, call, jobs=False):
    """every pattern of the size through `call` (input -> (error, out)); the patterns that came back wrong"""
    bad = []
    for name, x in sc.patterns(LIM, width, n, jobs):
        rc, out = call(x)
        why = "error %d" % rc if rc != 0 else sc.mismatch(out, x, name)
        if why:
            bad.append("%s: %s" % (name, why))
    return bad


# ---- launch_scan / launch_scan64

@pytest.mark.parametrize("n", sc.scan_sizes(LIM))
@pytest.mark.parametrize("kind", sorted(WIDTHS))
def test_scan_at_every_seam(kind, n):
    assert failures(WIDTHS[kind], n, sc.scan) == []


@pytest.mark.parametrize("kind", sorted(WIDTHS))
def test_scan_of_nothing_writes_nothing(kind):
    rc, out = sc.scan(np.zeros(0, sc.dtype_of(WIDTHS[kind])))
    assert rc == 0 and len(out) == sc.guard() and (out == np.uint64(sc.FILL)).all()


@pytest.mark.parametrize("kind", sorted(WIDTHS))
def test_scan_refuses_temporary_storage_that_is_too_small(kind):
    """The launcher needs one word per tile and refuses less, before any launch; scan_temp_bytes asks for that and one word to spare."""
    p, w, t, s = sc.seams(LIM)
    for n in (1, t, t + 1, 3 * t, s + 1):
        tiles = (n + t - 1) // t
        x = dict(sc.patterns(LIM, WIDTHS[kind], n))["random"]
        assert 8 * tiles <= sc.scan_temp_bytes(n) <= 8 * (tiles + 1)
        rc, out = sc.scan(x, temp_bytes=8 * tiles - 8)
        assert rc == sc.INVALID_VALUE and (out == np.uint64(sc.FILL)).all(), n
        rc, out = sc.scan(x, temp_bytes=8 * tiles - 1)
        assert rc == sc.INVALID_VALUE and (out == np.uint64(sc.FILL)).all(), n
        rc, out = sc.scan(x, temp_bytes=8 * tiles)
        assert rc == 0 and sc.mismatch(out, x, "exactly enough") is None, n


@pytest.mark.parametrize("kind", sorted(WIDTHS))
def test_two_scans_give_the_same_bytes(kind):
    for n in sc.scan_sizes(LIM):
        x = dict(sc.patterns(LIM, WIDTHS[kind], n))["random"]
        (r1, o1), (r2, o2) = sc.scan(x), sc.scan(x)
        assert r1 == 0 and r2 == 0 and o1.tobytes() == o2.tobytes(), n


# ---- launch_scan_jobs

@pytest.mark.parametrize("n", sc.job_sizes(LIM))
@pytest.mark.parametrize("kind", sorted(WIDTHS))
def test_one_job_at_every_seam(kind, n):
    def call(x):
        rc, outs = sc.scan_jobs([(x, None)])
        return rc, outs[0]
    assert failures(WIDTHS[kind], n, call, jobs=True) == []
    if n == 0:
        rc, outs = sc.scan_jobs([(np.zeros(0, sc.dtype_of(WIDTHS[kind])), None)])
        assert rc == 0 and (outs[0] == np.uint64(sc.FILL)).all()


def job_input(width, n, seed):
    """full-range values that wrap a 64-bit sum where the type can"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << (8 * width), n, dtype=np.uint64, endpoint=False).astype(sc.dtype_of(width))


def test_one_to_six_jobs_in_one_launch():
    """Jobs of different sizes and kinds side by side, an empty one between two that are not: every workgroup sums its own job and nothing else."""
    t = LIM.tile
    sizes = [4 * t + 1, 0, 257, t, 8 * t + 5, 3]
    assert len(sizes) == LIM.max_jobs
    for count in range(1, LIM.max_jobs + 1):
        for flip in (0, 1):
            xs = [job_input(8 if (k + flip) % 2 else 4, sizes[k], 40 + 10 * count + k) for k in range(count)]
            rc, outs = sc.scan_jobs([(x, None) for x in xs])
            assert rc == 0
            for k, (x, out) in enumerate(zip(xs, outs)):
                assert sc.mismatch(out, x, "job %d of %d" % (k, count)) is None
    rc, outs = sc.scan_jobs([])                                          # no job: no launch
    assert rc == 0 and outs == []


@pytest.mark.parametrize("kind", sorted(WIDTHS))
def test_a_job_whose_length_is_on_the_device(kind):
    """n = *n_dev + j.n, read by the kernel: the sum runs over both parts as one array."""
    for n_dev, n in sc.n_dev_pairs(LIM):
        for pattern in ("ones", "random"):
            x = dict(sc.patterns(LIM, WIDTHS[kind], n_dev + n))[pattern]
            rc, outs = sc.scan_jobs([(x, n_dev)])
            assert rc == 0 and sc.mismatch(outs[0], x, (n_dev, n, pattern)) is None
    # beside a job whose length the host knows, and an empty one with a device word of zero
    t = LIM.tile
    xs = [job_input(WIDTHS[kind], t + 1, 7), job_input(4, 0, 8), job_input(8, 4 * t + 5, 9)]
    rc, outs = sc.scan_jobs([(xs[0], t), (xs[1], 0), (xs[2], None)])
    assert rc == 0 and [sc.mismatch(o, x, k) for k, (x, o) in enumerate(zip(xs, outs))] == [None] * 3


# ---- launch_offsets_rebase

@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_offsets_rebase(n):
    """out[i] = base + local[i] mod 2^64; sub_batch passes base = 0 - offsets[first], so that every sum wraps back to a small number."""
    rng = np.random.default_rng(n)
    o0 = 0x123456789ABC
    local = np.sort(rng.integers(0, 1 << 40, n, dtype=np.uint64)) + np.uint64(o0)
    for base in ((1 << 64) - o0, 0, 977, (1 << 64) - 1):
        rc, out = sc.offsets_rebase(local, n, base)
        exp = ((local.astype(object) + base) % (1 << 64)).astype(np.uint64) if n else np.zeros(0, np.uint64)
        assert rc == 0 and out[:n].tolist() == exp.tolist() and (out[n:] == np.uint64(sc.FILL)).all(), (n, base)
        rc, out = sc.offsets_rebase(None, n, base)                       # local null: zeros
        assert rc == 0 and (out[:n] == np.uint64(base)).all() and (out[n:] == np.uint64(sc.FILL)).all(), (n, base)
    if n:
        rc, out = sc.offsets_rebase(local, n, (1 << 64) - o0)
        assert out[:n].tolist() == (local - np.uint64(o0)).tolist() and int(out[:n].max()) < 1 << 40

"""ONE document beyond 4 GiB against the oracle on every route.  The reference folds one Text of any Int length (Automaton.hs:452, 468-480) and the ABI's
end_pos is a u64, but before this file no test put a position at or above 2^32 inside one haystack: test_gpu_large.py reaches 5 GiB only as a ragged batch
of haystacks of at most 2 MiB.  The code that only a long document meets mixes 64- and 32-bit offsets: k_dfa's walk in 32-bit offsets from a u64 base
(the clamp of he_r), k_dfa_place's end_pos, k_sf's positions written as two halves, the per-KiB haystack index whose 5 M entries all name haystack 0,
per-haystack u64 counts fed by 32-bit lane sums, am_run_range's rebase of a window's records.  A truncation to 32 bits in any of them passed the rest of
the suite.

  A  one 5-GiB haystack, every search route: cfg2's 10k needles (CaseSensitive, k_sf), cfg3's 100k (IgnoreCase, mixed text, k_sf), the 100k-word dictionary
     over natural text (IgnoreCase: the library's choice, k_dfa forced, k_sf forced).  Records against the oracle's full lists on ~30 spread 1-MiB windows,
     the bytes around 2^32 and the last 32 MiB; the whole document's count against the oracle's (all 5 GiB, on 16 threads); every route's records equal to
     those of k_ac (the tests' second algorithm, itself held to the oracle on the same windows) record for record in HBM; which kernels ran is read from the
     library's launch profile.  containsAny with one needle in 5 GiB, after 2^32 and before it.
  B  am_run_range / am_count_range over the 5-GiB host slice: cuts at 2^32 - 1, 2^32, 2^32 + 1 and inside code points past 2^32.
  C  more than 2^32 values and records in one haystack: 5 GiB of `a` against {a, aa, aaa}.

Locality (why an oracle window with a warm-up is the whole document's answer there): the reference's state after a position is that of the longest suffix of
the text read so far that is a prefix of some needle (Automaton.hs:482-534: the fold follows goto edges and, where there is none, fallback edges, and a
fallback only ever shortens that suffix).  That suffix is never longer than the longest needle, so the state after byte p -- and so the matches reported
there -- depends only on the last (longest needle) code points before p, at most 4 bytes each.  A scan started `warm` = 4 x (longest needle in code points)
+ 16 bytes earlier, on a code point boundary, reports from there on exactly what the whole scan reports.  test_run_range_partitions_equal_the_whole_scan and
am_run_range rely on the same."""
import ctypes as C
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import alfred_margaret_amd as am
from alfred_margaret_amd import synth
from oracle import oracle
from tests.test_gpu_large import GIB5, spread

pytestmark = pytest.mark.gpu

TWO32 = 1 << 32
THREADS = 16                 # the parallel oracle
KELVIN = "K"            # KELVIN SIGN: three bytes, lowers to the one-byte k


def _lib():
    lib = am.api.libam()
    lib.am_matches_device_data.restype = C.c_void_p
    return lib


def _cont(x):
    return 0x80 <= x < 0xC0


def _boundary(host, x):
    """x moved forward onto a code point boundary"""
    while x < len(host) and _cont(host[x]):
        x += 1
    return x


def _back(host, x):
    """x moved back onto a code point boundary"""
    while x > 0 and _cont(host[x]):
        x -= 1
    return x


def warm_of(needles):
    return 4 * max(len(n) for n in needles) + 16


class _DevArray:
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "strides": None, "version": 2}


def records_view(m):
    """The records of a device-resident result as an int64 [n, 2] torch view of HBM (column 0: end_pos; column 1: haystack | state << 32); no copy."""
    import torch
    lib = _lib()
    n = int(lib.am_matches_size(m))
    p = lib.am_matches_device_data(m)
    assert p, "result not in HBM"
    return torch.as_tensor(_DevArray(p, 2 * n), device="cuda:0").view(n, 2)


def _end_pos_at(m, i):
    r = np.zeros(1, am.api.MATCH_DTYPE)
    am.check(_lib().am_matches_copy(m, C.c_uint64(i), C.c_uint64(1), r.ctypes.data))
    return int(r["end_pos"][0])


def first_after(m, x):
    """index of the first record of a one-haystack result with end_pos > x (binary search, one record copied per step)"""
    lo, hi = 0, int(_lib().am_matches_size(m))
    while lo < hi:
        mid = (lo + hi) // 2
        if _end_pos_at(m, mid) <= x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def copy_records(m, i, j):
    out = np.zeros(j - i, am.api.MATCH_DTYPE)
    if j > i:
        am.check(_lib().am_matches_copy(m, C.c_uint64(i), C.c_uint64(j - i), out.ctypes.data))
    return out


def expand(rs, vo, vals):
    """records -> the (matchPos, value) sequence the reference's fold sees"""
    st = rs["state"].astype(np.int64)
    lens = (vo[st + 1] - vo[st]).astype(np.int64)
    pos = np.repeat(rs["end_pos"].astype(np.uint64), lens)
    val = np.concatenate([vals[int(vo[x]):int(vo[x + 1])] for x in st]) if len(rs) else np.zeros(0, np.uint32)
    return pos, val


def oracle_window(o, case, host, lo, hi, warm):
    """the oracle's (matchPos, value) of the whole document with lo < matchPos <= hi, from a scan that starts `warm` bytes before lo"""
    s = _back(host, max(0, lo - warm))
    pos, val = o.run_list(case, host, off=s, length=hi - s)
    pos = pos.astype(np.uint64) + np.uint64(s)
    keep = pos > np.uint64(lo)
    return pos[keep], val[keep]


def oracle_count(o, case, host, warm, piece=64 << 20):
    """countMatches of the whole document: per piece (s, e] the count of a scan from s - warm to e minus that of the same scan to s; 16 threads"""
    n = len(host)
    cuts = sorted({0, n} | {_boundary(host, x) for x in range(piece, n, piece)})

    def one(k):
        s, e = cuts[k], cuts[k + 1]
        if s == 0:
            return o.count_matches(case, host, 0, e)
        b = _back(host, s - warm)
        return o.count_matches(case, host, b, e - b) - o.count_matches(case, host, b, s - b)
    with ThreadPoolExecutor(THREADS) as pool:
        return sum(pool.map(one, range(len(cuts) - 1)))


def plant(text, n, at, data):
    """write `data` (whole code points) at bytes [at, at + len) of the device document of n bytes; the pieces of the code points it cuts on either side become spaces"""
    import torch
    e = at + len(data)
    assert 4 <= at and e <= n
    w0, w1 = at - 4, min(e + 4, n)
    win = bytearray(text[w0:w1].cpu().numpy().tobytes())
    i = at - w0
    if _cont(win[i]):
        j = i - 1
        while j > 0 and _cont(win[j]):
            j -= 1
        win[j:i] = b" " * (i - j)
    k = e - w0
    while k < len(win) and _cont(win[k]):
        win[k] = 0x20
        k += 1
    win[i:e - w0] = data
    text[w0:w1] = torch.frombuffer(win, dtype=torch.uint8).to(text.device)


def chain(needles):
    """bytes S at whose last three positions needles end: a needle, then twice one byte that completes another needle"""
    nb = [x.encode() for x in needles if x]
    by_init = {}
    for y in nb:
        by_init.setdefault(y[:-1], y)
    longest = max(len(y) for y in nb)
    for x in sorted(nb, key=len):
        s = x
        for _ in range(2):
            for k in range(min(len(s), longest), -1, -1):
                y = by_init.get(s[len(s) - k:])
                if y is not None:
                    s += y[-1:]
                    break
            else:
                break
        else:
            return s
    raise AssertionError("no chain of three needle ends in this needle set")


def kernel_launches(names=("sf", "dfa", "dfa_place", "ac")):
    lib = _lib()
    out = {}
    for k in names:
        ms, nl = C.c_double(0), C.c_uint64(0)
        am.check(lib.am_profile_read(k.encode(), C.byref(ms), C.byref(nl)))
        out[k] = int(nl.value)
    return out


def run_profiled(a, case, b, kernel):
    import torch
    lib = _lib()
    a.set_kernel(kernel)
    am.check(lib.am_profile_reset()); am.check(lib.am_profile_enable(1))
    m = C.c_void_p()
    try:
        am.check(lib.am_run_batch(a.device, case, b, C.byref(m)))
        torch.cuda.synchronize()
    finally:
        lib.am_profile_enable(0)
    return m, kernel_launches()


def expect_route(kernel, uses_dfa, launched):
    """the kernels route `kernel` launched (am_profile_read), not what set_kernel asked for"""
    if kernel == 1:
        assert launched["ac"] >= 1 and launched["sf"] == launched["dfa"] == 0, launched
    elif uses_dfa:
        assert launched["dfa"] >= 1 and launched["dfa_place"] >= 1 and launched["sf"] == launched["ac"] == 0, launched
    else:
        assert launched["sf"] >= 1 and launched["dfa"] == launched["dfa_place"] == launched["ac"] == 0, launched


def make_document(workload):
    import torch
    w = synth.WORKLOADS[workload]
    needles = synth.needles_for(workload)
    text, n = synth.haystacks_device(needles, w["mixed"], 0, GIB5 // synth.CELL, torch.device("cuda:0"), natural=bool(w.get("natural")))
    assert n == GIB5
    return w, needles, text, n


def plant_edges(text, n, needles, kelvin):
    """needles placed where the reference must report matches at the 4-GiB edge and at the document's end; returns those end positions.
    kelvin=False: needle ends at 2^32 - 1, 2^32 and 2^32 + 1 (the last needle starts before byte 2^32 and ends after it); kelvin=True (IgnoreCase): a needle
    with a K (KELVIN SIGN, lowers to k) at bytes [2^32 - 1, 2^32 + 2), one code point across the edge."""
    want = []
    if not kelvin:
        s = chain(needles)
        plant(text, n, TWO32 + 1 - len(s), s)
        want += [TWO32 - 1, TWO32, TWO32 + 1]
    else:
        x = next(x for x in sorted(needles, key=len) if "k" in x[1:])
        j = x.index("k", 1)
        t = (x[:j] + KELVIN + x[j + 1:]).encode()
        at = TWO32 - 1 - len(x[:j].encode())
        plant(text, n, at, t)
        want.append(at + len(t))
    last = min((x for x in needles if x), key=len).encode()
    plant(text, n, n - len(last), last)
    want.append(n)
    return want


def check_document(workload, routes, kelvin=False):
    """A: one 5-GiB haystack of `workload`'s text; routes = [(kernel, takes k_dfa)]"""
    import torch
    w, needles, text, n = make_document(workload)
    case = w["case"]
    want = plant_edges(text, n, needles, kelvin)
    host_t = torch.empty(n, dtype=torch.uint8)
    host_t.copy_(text[:n])
    host = host_t.numpy()
    a, o = am.Automaton(needles), oracle.Machine(needles)
    vo, vals = a.values_off(), a.values()
    warm = warm_of(needles)
    # the windows: 1-MiB pieces spread over the document (the first, the last, those around 2^32), the bytes right around 2^32, the last 32 MiB
    mib = np.arange(0, n + 1, 1 << 20, dtype=np.int64)
    wins = [(int(mib[i]), int(mib[i + 1])) for i in spread(mib, 30)] + [(TWO32 - 4096, TWO32 + 4096), (n - (32 << 20), n)]
    wins = [(_boundary(host, lo), _boundary(host, hi)) for lo, hi in wins]
    with ThreadPoolExecutor(THREADS) as pool:
        exp = list(pool.map(lambda lh: oracle_window(o, case, host, lh[0], lh[1], warm), wins))
    exp_count = oracle_count(o, case, host, warm)
    assert np.isin(np.asarray(want, np.uint64), np.concatenate([e[0] for e in exp])).all(), (workload, "planted ends", want)
    lib = _lib()
    offs = torch.tensor([0, n], dtype=torch.int64, device=text.device)
    b = C.c_void_p()
    am.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), 1, n, C.byref(b)))
    ref, m = C.c_void_p(), None
    try:
        ref, launched = run_profiled(a, case, b, 1)               # k_ac: the second algorithm, itself held to the oracle below like the others
        expect_route(1, False, launched)
        ref_v = records_view(ref)
        for kernel, uses_dfa in [(1, False)] + list(routes):
            if kernel == 1:
                m = ref
            else:
                m, launched = run_profiled(a, case, b, kernel)
                expect_route(kernel, uses_dfa, launched)
            size = int(lib.am_matches_size(m))
            for (lo, hi), (pos, val) in zip(wins, exp):
                rs = copy_records(m, first_after(m, lo), first_after(m, hi))
                gpos, gval = expand(rs, vo, vals)
                assert np.array_equal(gpos, pos) and np.array_equal(gval, val), (workload, kernel, "window", lo, hi, len(gpos), len(pos))
                assert (rs["haystack"] == 0).all()
            assert _end_pos_at(m, size - 1) == n
            if m is not ref:
                assert size == int(lib.am_matches_size(ref)) and torch.equal(records_view(m), ref_v), (workload, kernel, "records differ from k_ac's")
                lib.am_matches_free(m)
            m = None
            counts, tot = np.zeros(1, np.uint64), C.c_uint64(0)
            am.check(lib.am_count_batch(a.device, case, b, counts.ctypes.data, C.byref(tot)))
            assert int(counts[0]) == tot.value == exp_count, (workload, kernel, int(counts[0]), tot.value, exp_count)
        a.set_kernel(0)
        sl = am.api.Slice(host.ctypes.data, 0, n)
        c = np.zeros(1, np.uint64)
        am.check(lib.am_count(a.device, case, C.byref(sl), 1, c.ctypes.data))
        assert int(c[0]) == exp_count, (workload, "am_count", int(c[0]), exp_count)
    finally:
        a.set_kernel(0)
        if m is not None and m is not ref:
            lib.am_matches_free(m)
        if ref.value:
            lib.am_matches_free(ref)
        lib.am_batch_destroy(b)
        lib.am_release_device_memory()
    return len(wins)


def test_one_5gib_document_of_cfg2_on_the_suffix_filter():
    assert check_document("cfg2_runText_10k_1GiB", routes=[(2, False)]) >= 30


def test_one_5gib_document_of_cfg3_ignore_case_on_the_suffix_filter():
    assert check_document("cfg3_runLower_100k_10GiB", routes=[(2, False)], kelvin=True) >= 30


def test_one_5gib_document_of_the_dictionary_on_every_route():
    # 0: the library's own choice (the sample walk sends a dictionary over its language to k_dfa), 3: the table walk forced, 2: the suffix filter forced
    assert check_document("natural_100k_10GiB", routes=[(0, True), (3, True), (2, False)]) >= 30


def test_contains_any_finds_the_one_needle_of_a_5gib_document():
    """cfg2's automaton over 5 GiB of a byte no needle contains and ONE needle: after 2^32, then (alone) before it -- flag, count and the record's end_pos on every route."""
    import torch
    needles = synth.needles_for("cfg2_runText_10k_1GiB")
    a, o = am.Automaton(needles), oracle.Machine(needles)
    fill = b"~"
    assert not any(fill.decode() in x for x in needles)
    x = next(x.encode() for x in needles if o.count_matches(0, fill * 8 + x.encode() + fill * 8) == 1)    # no other needle inside it
    n = GIB5
    text = torch.full((n + 64,), fill[0], dtype=torch.uint8, device="cuda:0")
    text[n:] = 0
    offs = torch.tensor([0, n], dtype=torch.int64, device="cuda:0")
    lib = _lib()
    b = C.c_void_p()
    am.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), 1, n, C.byref(b)))
    try:
        for at in (TWO32 + 1000, TWO32 - len(x)):                 # all of it past 2^32; all of it before (its last byte is byte 2^32 - 1)
            text[:n] = fill[0]
            text[at:at + len(x)] = torch.frombuffer(bytearray(x), dtype=torch.uint8).to(text.device)
            for kernel in (0, 2, 1):
                a.set_kernel(kernel)
                flags = np.zeros(1, np.uint8)
                am.check(lib.am_contains_any_batch(a.device, 0, b, flags.ctypes.data))
                counts, tot = np.zeros(1, np.uint64), C.c_uint64(0)
                am.check(lib.am_count_batch(a.device, 0, b, counts.ctypes.data, C.byref(tot)))
                m = C.c_void_p()
                am.check(lib.am_run_batch(a.device, 0, b, C.byref(m)))
                try:
                    rs = am.api.matches_to_numpy(m)
                finally:
                    lib.am_matches_free(m)
                assert int(flags[0]) == 1 and int(counts[0]) == tot.value == 1, (at, kernel, int(flags[0]), int(counts[0]))
                assert len(rs) == 1 and int(rs["end_pos"][0]) == at + len(x) and int(rs["haystack"][0]) == 0, (at, kernel, rs)
    finally:
        a.set_kernel(0)
        lib.am_batch_destroy(b)


def test_run_range_partitions_one_5gib_document():
    """B: am_run_range / am_count_range over the 5-GiB host slice of cfg3's document (IgnoreCase; a K across byte 2^32): cuts at 2^32 - 1, 2^32, 2^32 + 1 (inside
    the K), inside another code point past 2^32 and at random places.  The ranges' records concatenated are the whole scan's (am_run_batch, which part A holds
    to the oracle), their counts add up to its count; a range above 2^32 against the oracle directly; hi = len + 1 is refused."""
    import torch
    w, needles, text, n = make_document("cfg3_runLower_100k_10GiB")
    case = w["case"]
    plant_edges(text, n, needles, kelvin=True)
    host_t = torch.empty(n, dtype=torch.uint8)
    host_t.copy_(text[:n])
    host = host_t.numpy()
    a, o = am.Automaton(needles), oracle.Machine(needles)
    vo, vals = a.values_off(), a.values()
    lib = _lib()
    offs = torch.tensor([0, n], dtype=torch.int64, device=text.device)
    b = C.c_void_p()
    am.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), 1, n, C.byref(b)))
    whole = C.c_void_p()
    sl = am.api.Slice(host.ctypes.data, 0, n)
    try:
        a.set_kernel(0)
        am.check(lib.am_run_batch(a.device, case, b, C.byref(whole)))
        total = C.c_uint64(0)
        am.check(lib.am_count_batch(a.device, case, b, None, C.byref(total)))
        lead = TWO32 + (1 << 20) + int(np.argmax(host[TWO32 + (1 << 20):TWO32 + (2 << 20)] >= 0xC0))
        assert host[lead] >= 0xC0
        rng = random.Random(32)
        cuts = sorted({0, n, TWO32 - 1, TWO32, TWO32 + 1, lead + 1} | {rng.randrange(1, n) for _ in range(4)})
        counted = 0
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            m = C.c_void_p()
            am.check(lib.am_run_range(a.device, case, C.byref(sl), lo, hi, C.byref(m)))
            try:
                part = am.api.matches_to_numpy(m)
            finally:
                lib.am_matches_free(m)
            ref = copy_records(whole, first_after(whole, lo), first_after(whole, hi))
            assert len(part) == len(ref) and part.tobytes() == ref.tobytes(), ("range", lo, hi, len(part), len(ref))
            c = C.c_uint64(0)
            am.check(lib.am_count_range(a.device, case, C.byref(sl), lo, hi, C.byref(c)))
            assert c.value == int(np.diff(vo)[part["state"].astype(np.int64)].sum()), ("count of range", lo, hi)
            counted += c.value
        assert counted == total.value
        lo, hi = TWO32 + 3, _boundary(host, TWO32 + (8 << 20))
        m = C.c_void_p()
        am.check(lib.am_run_range(a.device, case, C.byref(sl), lo, hi, C.byref(m)))
        try:
            gpos, gval = expand(am.api.matches_to_numpy(m), vo, vals)
        finally:
            lib.am_matches_free(m)
        pos, val = oracle_window(o, case, host, lo, hi, warm_of(needles))
        assert len(pos) > 0 and np.array_equal(gpos, pos) and np.array_equal(gval, val), (len(gpos), len(pos))
        m = C.c_void_p()
        assert lib.am_run_range(a.device, case, C.byref(sl), 5, n + 1, C.byref(m)) == am.AM_ERR_INVALID
    finally:
        a.set_kernel(0)
        if whole.value:
            lib.am_matches_free(whole)
        lib.am_batch_destroy(b)
        lib.am_release_device_memory()


def _document_of(byte, n):
    import torch
    text = torch.full((n + 64,), byte, dtype=torch.uint8, device="cuda:0")
    text[n:] = 0
    offs = torch.tensor([0, n], dtype=torch.int64, device="cuda:0")
    b = C.c_void_p()
    am.check(_lib().am_batch_from_device(text.data_ptr(), offs.data_ptr(), 1, n, C.byref(b)))
    return text, offs, b


def _count_batch(a, case, b):
    counts, tot = np.zeros(1, np.uint64), C.c_uint64(0)
    rc = _lib().am_count_batch(a.device, case, b, counts.ctypes.data, C.byref(tot))
    return rc, int(counts[0]), tot.value


def test_more_than_2_32_values_in_one_haystack_are_counted():
    """C.1: 5 GiB of `a` (CaseSensitive) / `A` (IgnoreCase) against {a, aa, aaa}: 3n - 3 values (the oracle pins the closed form on 1 MiB), counted on k_sf and
    k_dfa; {"", "a"} (the dense route) counted exactly, or refused cleanly and then counted in ranges."""
    import torch
    n = GIB5
    lib = _lib()
    for case, ch in ((am.CASE_SENSITIVE, b"a"), (am.IGNORE_CASE, b"A")):
        o = oracle.Machine(["a", "aa", "aaa"])
        assert o.count_matches(case, ch * (1 << 20)) == 3 * (1 << 20) - 3
        a = am.Automaton(["a", "aa", "aaa"])
        text, offs, b = _document_of(ch[0], n)
        try:
            for kernel, name in ((2, "sf"), (3, "dfa")):
                a.set_kernel(kernel)
                am.check(lib.am_profile_reset()); am.check(lib.am_profile_enable(1))
                try:
                    rc, c, tot = _count_batch(a, case, b)
                    torch.cuda.synchronize()
                finally:
                    lib.am_profile_enable(0)
                am.check(rc)
                assert kernel_launches((name,))[name] >= 1, (case, kernel)
                assert c == tot == 3 * n - 3 > TWO32, (case, kernel, c, tot)
        finally:
            a.set_kernel(0)
            lib.am_batch_destroy(b)
            del text
    # the dense route: the empty needle ends at every position
    o = oracle.Machine(["", "a"])
    k = 1 << 20
    c1, c2, c3 = (o.count_matches(0, b"a" * x) for x in (k, k + 1, k + 7))
    slope = c2 - c1
    assert c3 == c1 + 7 * slope
    expect = c1 + slope * (n - k)
    a = am.Automaton(["", "a"])
    text, offs, b = _document_of(ord("a"), n)
    try:
        rc, c, tot = _count_batch(a, 0, b)
    finally:
        lib.am_batch_destroy(b)
        del text
    if rc == am.AM_OK:
        assert c == tot == expect, (c, tot, expect)
    else:
        assert rc == am.AM_ERR_UNSUPPORTED and lib.am_last_error(), rc
        host = np.full(n, ord("a"), np.uint8)
        sl = am.api.Slice(host.ctypes.data, 0, n)
        got, step = 0, 1 << 30
        for lo in range(0, n, step):
            cnt = C.c_uint64(0)
            am.check(lib.am_count_range(a.device, 0, C.byref(sl), lo, min(n, lo + step), C.byref(cnt)))
            got += cnt.value
        assert got == expect, (got, expect)


def test_more_than_2_32_records_in_one_haystack():
    """C.2: 5 GiB of `a` against {a, aa, aaa} has a record at every byte, 5.4 G of them.  k_sf addresses record slots with 32 bits and must refuse (AM_ERR_UNSUPPORTED,
    no result).  k_dfa's tokens carry (unit ordinal, lane, sequence in the unit) inside a superblock whose first unit group is kept apart, and k_dfa_place puts a
    record at unit_offsets[u] + sequence, all of it in 64 bits (unit counts are u32, but a unit is at most 8 KiB): its records are checked in HBM against the
    closed form -- end_pos = i + 1, haystack 0, the state of `a`, of `aa`, then that of `aaa` -- whose values the oracle gives."""
    import torch
    n = GIB5
    lib = _lib()
    needles = ["a", "aa", "aaa"]
    a, o = am.Automaton(needles), oracle.Machine(needles)
    vo, vals = a.values_off(), a.values()
    opos, oval = o.run_list(0, b"aaa")
    text, offs, b = _document_of(ord("a"), n)
    m = C.c_void_p()
    try:
        a.set_kernel(2)
        rc = lib.am_run_batch(a.device, 0, b, C.byref(m))
        assert rc == am.AM_ERR_UNSUPPORTED and not m.value, (rc, m.value)
        assert b"2^32" in (lib.am_last_error() or b"")
        free, _ = torch.cuda.mem_get_info()
        need = 16 * n + 13 * n + (4 << 30)                        # records + the token pool (8 bytes per token, 3 072 of a superblock's 4 096 slots used) + room
        if free < need:
            pytest.skip("%.0f GB of device memory free, %.0f GB needed for 5.4 G records and their tokens" % (free / 1e9, need / 1e9))
        a.set_kernel(3)
        am.check(lib.am_profile_reset()); am.check(lib.am_profile_enable(1))
        try:
            am.check(lib.am_run_batch(a.device, 0, b, C.byref(m)))
            torch.cuda.synchronize()
        finally:
            lib.am_profile_enable(0)
        launched = kernel_launches()
        assert launched["dfa"] >= 1 and launched["dfa_place"] >= 1, launched
        size = int(lib.am_matches_size(m))
        assert size == n > TWO32
        head = copy_records(m, 0, 3)
        gpos, gval = expand(head, vo, vals)
        assert np.array_equal(gpos, opos) and np.array_equal(gval, oval), (head, opos, oval)
        v = records_view(m)
        word = int(head["state"][2]) << 32                        # haystack 0 in the low half
        step = 1 << 28
        for i in range(0, size, step):
            j = min(size, i + step)
            blk = v[i:j]
            assert torch.equal(blk[:, 0], torch.arange(i + 1, j + 1, dtype=torch.int64, device=blk.device)), ("end_pos", i)
            s = max(i, 3) - i
            assert bool((blk[s:, 1] == word).all()), ("state / haystack", i)
        assert _end_pos_at(m, size - 1) == n
    finally:
        a.set_kernel(0)
        if m.value:
            lib.am_matches_free(m)
        lib.am_batch_destroy(b)
        del text
        lib.am_release_device_memory()

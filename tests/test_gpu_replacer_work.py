"""The pass-by-pass Replacer loops (csrc/am_replacer.cpp: replacer_run splices the texts, replacer_run_pt keeps them as piece tables) do the SAME WORK on every
route, not only return the right text: per case a fresh replacer, one warm call, then one call between am_profile_reset / am_profile_enable(1) and am_profile_read
on an uploaded batch (the raw ABI, as tests/measure/replacer_bench.py).  Held: the texts and Nothing entries (= the oracle's Replacer.run, exactly), the passes,
the bytes scanned and spliced, and the launches per profile name.

EXPECTED holds what commit 3c885b7 (the parent of the change that gave both loops one pass skeleton) did, read there on an MI355X, twice with the same figures;
no name had to be left out.  A profile bracket (`Prof`) counts once per step of a pass, whatever the step launches: the bookkeeping sums of a pass are ONE
`rp_scans` whether k_scan_jobs does them in one launch or, beyond 2^18 haystacks, a scan launch per sum.  What the counts do show is how many loops saw the
haystacks: input D (2^18 + 1 500 haystacks) under AM_RP_GROUPS=1 has rp_scans == passes -- one loop, whose first pass has n_act + 1 > 2^18 and so, by
scan_pass's rule (read from the code, not shown by a count), takes the multi-launch branch of the sums and of the window-length scan -- where the default two groups (what test_replacer_many_tiny_haystacks_large_bookkeeping runs:
about 131 800 haystacks each, both below 2^18) give twice that.

The four switches that are read once per process (AM_RP_NO_FUSE, AM_RP_NO_SPIN, AM_RP_MAT_MAIN, AM_RP_NO_RANGE_REUSE) stay with tests/measure/replacer_toggles.py."""
import ctypes as C
import functools
import json
import random

import pytest

import alfred_margaret_amd as am
from oracle import oracle

pytestmark = pytest.mark.gpu

NAMES = ("rp_ranges", "rp_pass", "rp_scans", "rp_route", "rp_splice", "rp_windows", "rp_merge", "pt_build", "pt_materialise", "hidx", "sf", "ac", "scan", "permute")

INC = {"AM_RP_LOOP": 0}
FULL = {"AM_RP_LOOP": 0, "AM_RP_FULL_SCANS": 1}
PIECES = {"AM_RP_LOOP": 0, "AM_RP_PIECES": 1}
PF = {"AM_RP_LOOP": 0, "AM_RP_PARALLEL_FOLD": 1}
PF_PIECES = {"AM_RP_LOOP": 0, "AM_RP_PARALLEL_FOLD": 1, "AM_RP_PIECES": 1}
GROUPS3 = {"AM_RP_LOOP": 0, "AM_RP_GROUPS": 3}
# (which loop AM_RP_LOOP=0 alone reaches follows from the batch: 64 haystacks or more of at most 1 MiB each and a CaseSensitive replacer -- input B under case 0 -- go
# to the piece-table loop, everything else to the splicing loop)
ROUTES = {"inc": (0, INC), "inc_ic": (1, INC), "full": (0, FULL), "pieces": (0, PIECES), "pf": (0, PF), "pf_pieces": (0, PF_PIECES), "groups3": (0, GROUPS3)}
ROUTES_IC = {"inc": (1, INC), "full": (1, FULL), "pf": (1, PF), "groups3": (1, GROUPS3)}           # input C: the piece-table loop is CaseSensitive only
# (input D under case 1: the splicing loop with its windows, whose lengths are summed by a launch of their own beyond 2^18 haystacks)
ROUTES_D = {"full": (0, {"AM_RP_LOOP": 0, "AM_RP_GROUPS": 1, "AM_RP_FULL_SCANS": 1}), "pieces": (0, {"AM_RP_LOOP": 0, "AM_RP_GROUPS": 1, "AM_RP_PIECES": 1}),
            "inc_ic": (1, {"AM_RP_LOOP": 0, "AM_RP_GROUPS": 1})}


@functools.lru_cache(maxsize=None)
def _input(name):
    """(pairs, haystacks) of an input; D's haystacks are ten distinct texts repeated"""
    if name == "A":
        return [("ab", "X"), ("Xc", "abab"), ("ba", ""), ("aX", "yy")], ["abcabcab" * 50, "ab", "bab", "", "cab" * 200]
    if name == "B":
        rng = random.Random(16)
        alpha = "abcde "
        pairs = [("".join(rng.choice(alpha) for _ in range(rng.randint(2, 4))), "".join(rng.choice("ABC" + alpha) for _ in range(rng.randint(0, 5)))) for _ in range(30)]
        hays = ["".join(rng.choice(alpha) for _ in range(rng.randint(2000, 6000))) for _ in range(2)]
        hays += ["".join(rng.choice(alpha) for _ in range(rng.randint(0, 30))) for _ in range(120)]
        rng.shuffle(hays)
        return pairs, hays
    if name == "C":
        return [("straße", "STR"), ("i", "İİ"), ("k", ""), ("å", "K")], ["Straße İstanbul KÅ" * 80, "strasse", "ẞ" * 50 + "straße"]
    assert name == "D"
    distinct = ["", "a", "ab", "abc", "cab", "abcab", "zzabzz", "bbbb", "Xc", "abab" * 3]
    n = (1 << 18) + 1500
    return [("ab", "X"), ("Xc", "ba"), ("b", "yy"), ("zz", "")], [distinct[(i * 7 + i // 11) % len(distinct)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def _expected_texts(name, case, max_len):
    """the oracle's answers, computed once per (input, case, limit) and shared by the routes"""
    pairs, hays = _input(name)
    o = oracle.Replacer(case, pairs)
    memo = {}
    for h in hays:
        if h not in memo:
            memo[h] = o.run(h, max_len)
    return [memo[h] for h in hays]


def _work(case, pairs, hays, max_len, switches):
    """(texts, (passes, scanned, spliced), launches per name) of the profiled second call of a fresh replacer under `switches`"""
    lib = am.api.libam()
    sl = am.api._Slices(hays)
    batch, res = C.c_void_p(), C.c_void_p()
    limit = C.c_uint64(2**64 - 1 if max_len < 0 else max_len)
    for k, v in switches.items():
        am.debug_set(k, v)
    try:
        r = am.Replacer(case, pairs)
        rdev = C.c_void_p(r.device)
        am.api.check(lib.am_batch_upload(sl.arr, sl.n, C.byref(batch)))
        am.api.check(lib.am_replacer_run_batch(rdev, batch, limit, C.byref(res)))          # warm: workspaces, pinned staging
        lib.am_replaced_free(res)
        res = C.c_void_p()
        am.api.check(lib.am_profile_reset())
        am.api.check(lib.am_profile_enable(1))
        try:
            am.api.check(lib.am_replacer_run_batch(rdev, batch, limit, C.byref(res)))
        finally:
            am.api.check(lib.am_profile_enable(0))
        launches = {}
        for k in NAMES:
            ms, n = C.c_double(0), C.c_uint64(0)
            am.api.check(lib.am_profile_read(k.encode(), C.byref(ms), C.byref(n)))
            if n.value:
                launches[k] = int(n.value)
        stats = (int(lib.am_replaced_passes(res)), int(lib.am_replaced_scanned_bytes(res)), int(lib.am_replaced_spliced_bytes(res)))
        assert int(lib.am_replaced_size(res)) == len(hays)
        texts = []
        p, n = C.c_void_p(), C.c_size_t(0)
        for i in range(len(hays)):
            just = lib.am_replaced_get(res, i, C.byref(p), C.byref(n))
            assert just >= 0
            texts.append(C.string_at(p, n.value) if just else None)
        return texts, stats, launches
    finally:
        for k in switches:
            am.debug_set(k, -1)
        if res:
            lib.am_replaced_free(res)
        if batch:
            lib.am_batch_destroy(batch)


def _hold(cid, name, case, max_len, switches):
    pairs, hays = _input(name)
    texts, stats, launches = _work(case, pairs, hays, max_len, switches)
    print("WORK " + json.dumps([cid, list(stats), launches]))
    exp = _expected_texts(name, case, max_len)
    bad = [i for i in range(len(hays)) if texts[i] != exp[i]]
    assert not bad, (cid, bad[:5], [texts[i] for i in bad[:5]])
    assert cid in EXPECTED, cid
    e_passes, e_scanned, e_spliced, e_launches = EXPECTED[cid]
    assert stats == (e_passes, e_scanned, e_spliced), (cid, "passes, bytes scanned, bytes spliced")
    assert launches == e_launches, (cid, "launches per profile name")
    return texts, stats, launches


@pytest.mark.parametrize("max_len", [-1, 40])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_input_a_several_passes_growth_deletion_limit(route, max_len):
    """Several passes, haystacks that finish in different passes, an empty haystack, growth and deletion; under the limit some, not all, become Nothing."""
    case, switches = ROUTES[route]
    texts, _, _ = _hold("A-%s-%d" % (route, max_len), "A", case, max_len, switches)
    if max_len >= 0:
        assert any(t is None for t in texts) and not all(t is None for t in texts)
    else:
        assert all(t is not None for t in texts)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_input_b_two_documents_among_many_tiny_ones(route):
    """Two long haystacks among 120 tiny ones: the piece-table loop switches between "windows + merge" and "materialise and scan whole"."""
    case, switches = ROUTES[route]
    _, _, launches = _hold("B-%s" % route, "B", case, -1, switches)
    assert ("pt_build" in launches) == (route in ("inc", "pieces", "pf", "pf_pieces", "groups3")), "which routes reach the piece-table loop"
    if "pt_build" in launches and route != "groups3":                # (in groups only one of the three is on the piece-table loop: its scans are not told apart from the others')
        # the first scan, a window scan before every merge at the most, and the rest: next texts materialised and scanned whole
        assert launches.get("rp_merge", 0) > 0, "windows + merge"
        assert launches["sf"] > 1 + launches["rp_merge"], "materialise and scan whole"


@pytest.mark.parametrize("route", sorted(ROUTES_IC))
def test_input_c_ignore_case_on_the_splicing_loop(route):
    """IgnoreCase with matches whose text is longer or shorter than the needle (ß / ẞ, İ, K / k, Å)."""
    case, switches = ROUTES_IC[route]
    _, _, launches = _hold("C-%s" % route, "C", case, -1, switches)
    assert launches.get("rp_splice", 0) > 0 and "pt_build" not in launches


@pytest.mark.parametrize("route", sorted(ROUTES_D))
def test_input_d_bookkeeping_beyond_one_scan_launch(route):
    """2^18 + 1 500 tiny haystacks in ONE loop (AM_RP_GROUPS=1).  What the counts show: one loop saw them all -- a bracket per pass, not per group and pass.
    That its first pass, with n_act + 1 > 2^18, takes the launch-per-sum branch of the bookkeeping sums and (piece tables, and the splicing loop under case 1)
    of the window-length sum is not shown by any count: it follows by scan_pass's and window_geometry's rule, read from the code."""
    case, switches = ROUTES_D[route]
    _, stats, launches = _hold("D-%s" % route, "D", case, -1, switches)
    assert launches["rp_scans"] == stats[0] and launches["rp_route"] == stats[0]
    assert launches.get("pt_build" if route == "pieces" else "rp_splice", 0) == stats[0]
    if route != "full":
        assert launches.get("rp_windows", 0) > 0, "window geometry"


# id -> (passes, bytes scanned, bytes spliced, launches per profile name), read on commit 3c885b7
EXPECTED = {
    "A-full--1": (4, 3060, 2212, {"hidx": 4, "permute": 4, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "scan": 4, "sf": 4}),
    "A-full-40": (2, 1008, 6, {"hidx": 2, "permute": 1, "rp_pass": 2, "rp_ranges": 2, "rp_route": 2, "rp_scans": 2, "rp_splice": 2, "scan": 2, "sf": 2}),
    "A-groups3--1": (4, 3060, 2212, {"hidx": 8, "permute": 8, "rp_pass": 8, "rp_ranges": 8, "rp_route": 8, "rp_scans": 8, "rp_splice": 8, "rp_windows": 8, "scan": 8, "sf": 8}),
    "A-groups3-40": (2, 1008, 6, {"hidx": 3, "permute": 2, "rp_pass": 3, "rp_ranges": 3, "rp_route": 3, "rp_scans": 3, "rp_splice": 3, "rp_windows": 2, "scan": 3, "sf": 3}),
    "A-inc--1": (4, 3060, 2212, {"hidx": 4, "permute": 4, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "rp_windows": 4, "scan": 4, "sf": 4}),
    "A-inc-40": (2, 1008, 6, {"hidx": 2, "permute": 1, "rp_pass": 2, "rp_ranges": 2, "rp_route": 2, "rp_scans": 2, "rp_splice": 2, "rp_windows": 1, "scan": 2, "sf": 2}),
    "A-inc_ic--1": (4, 3060, 2212, {"hidx": 4, "permute": 4, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "rp_windows": 4, "scan": 4, "sf": 4}),
    "A-inc_ic-40": (2, 1008, 6, {"hidx": 2, "permute": 1, "rp_pass": 2, "rp_ranges": 2, "rp_route": 2, "rp_scans": 2, "rp_splice": 2, "rp_windows": 1, "scan": 2, "sf": 2}),
    "A-pf--1": (4, 3060, 2212, {"hidx": 4, "permute": 4, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "rp_windows": 4, "scan": 4, "sf": 4}),
    "A-pf-40": (2, 1008, 6, {"hidx": 2, "permute": 1, "rp_pass": 2, "rp_ranges": 2, "rp_route": 2, "rp_scans": 2, "rp_splice": 2, "rp_windows": 1, "scan": 2, "sf": 2}),
    "A-pf_pieces--1": (4, 3060, 157, {"hidx": 4, "permute": 4, "pt_build": 4, "pt_materialise": 3, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_windows": 4, "scan": 4, "sf": 4}),
    "A-pf_pieces-40": (2, 1008, 3, {"hidx": 2, "permute": 2, "pt_build": 2, "pt_materialise": 2, "rp_merge": 1, "rp_pass": 2, "rp_ranges": 2, "rp_route": 2, "rp_scans": 2, "rp_windows": 3, "scan": 2, "sf": 2}),
    "A-pieces--1": (4, 3060, 157, {"hidx": 4, "permute": 4, "pt_build": 4, "pt_materialise": 3, "rp_pass": 4, "rp_route": 4, "rp_scans": 4, "rp_windows": 4, "scan": 4, "sf": 4}),
    "A-pieces-40": (2, 1008, 3, {"hidx": 2, "permute": 2, "pt_build": 2, "pt_materialise": 2, "rp_merge": 1, "rp_pass": 2, "rp_route": 2, "rp_scans": 2, "rp_windows": 3, "scan": 2, "sf": 2}),
    "B-full": (24, 209597, 211646, {"hidx": 24, "permute": 24, "rp_pass": 24, "rp_ranges": 24, "rp_route": 24, "rp_scans": 24, "rp_splice": 24, "scan": 24, "sf": 24}),
    "B-groups3": (24, 95186, 206675, {"hidx": 32, "permute": 32, "pt_build": 8, "pt_materialise": 8, "rp_merge": 19, "rp_pass": 32, "rp_ranges": 24, "rp_route": 32, "rp_scans": 32, "rp_splice": 24, "rp_windows": 51, "scan": 32, "sf": 32}),
    "B-inc": (24, 86459, 11804, {"hidx": 24, "permute": 24, "pt_build": 24, "pt_materialise": 10, "rp_merge": 20, "rp_pass": 24, "rp_route": 24, "rp_scans": 24, "rp_windows": 44, "scan": 24, "sf": 24}),
    "B-inc_ic": (24, 109144, 230060, {"hidx": 24, "permute": 24, "rp_merge": 15, "rp_pass": 24, "rp_ranges": 24, "rp_route": 24, "rp_scans": 24, "rp_splice": 24, "rp_windows": 39, "scan": 24, "sf": 24}),
    "B-pf": (24, 86459, 11804, {"hidx": 24, "permute": 24, "pt_build": 24, "pt_materialise": 10, "rp_merge": 20, "rp_pass": 24, "rp_ranges": 24, "rp_route": 24, "rp_scans": 24, "rp_windows": 44, "scan": 24, "sf": 24}),
    "B-pf_pieces": (24, 86459, 11804, {"hidx": 24, "permute": 24, "pt_build": 24, "pt_materialise": 10, "rp_merge": 20, "rp_pass": 24, "rp_ranges": 24, "rp_route": 24, "rp_scans": 24, "rp_windows": 44, "scan": 24, "sf": 24}),
    "B-pieces": (24, 86459, 11804, {"hidx": 24, "permute": 24, "pt_build": 24, "pt_materialise": 10, "rp_merge": 20, "rp_pass": 24, "rp_route": 24, "rp_scans": 24, "rp_windows": 44, "scan": 24, "sf": 24}),
    "C-full": (4, 6317, 5993, {"hidx": 4, "permute": 4, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "scan": 4, "sf": 4}),
    "C-groups3": (4, 6195, 5993, {"hidx": 6, "permute": 5, "rp_merge": 1, "rp_pass": 6, "rp_ranges": 6, "rp_route": 6, "rp_scans": 6, "rp_splice": 6, "rp_windows": 6, "scan": 6, "sf": 6}),
    "C-inc": (4, 6317, 5993, {"hidx": 4, "permute": 4, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "rp_windows": 4, "scan": 4, "sf": 4}),
    "C-pf": (4, 6317, 5993, {"hidx": 4, "permute": 4, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "rp_windows": 4, "scan": 4, "sf": 4}),
    "D-full": (4, 2089965, 1845504, {"hidx": 4, "permute": 3, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "scan": 4, "sf": 4}),
    "D-inc_ic": (4, 2089965, 1845504, {"hidx": 4, "permute": 3, "rp_pass": 4, "rp_ranges": 4, "rp_route": 4, "rp_scans": 4, "rp_splice": 4, "rp_windows": 3, "scan": 4, "sf": 4}),
    "D-pieces": (4, 2089965, 728615, {"hidx": 4, "permute": 4, "pt_build": 4, "pt_materialise": 4, "rp_merge": 2, "rp_pass": 4, "rp_route": 4, "rp_scans": 4, "rp_windows": 6, "scan": 4, "sf": 4}),
}

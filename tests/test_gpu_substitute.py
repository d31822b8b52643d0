"""Substitute on the device (am_substitute / am_substitute_batch / am_batch_substitute, csrc/am_subst.hip) against the definition.  Every check compares the bytes and
the offsets of the one-shot form, the batch form, the splice over a separately obtained spans result and the host mirror with what tests/substitute_reference.py says --
spans_reference over the oracle plus the splice, or literals -- never with another path of the library.  Shapes sit on the gather's real seams (am_substitute_geometry)."""
import ctypes as C
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, spans_reference as ref, substitute_reference as sref

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
KELVIN, ANGSTROM, SHARP_S, DOTTED_I = "\u212a", "\u212b", "\u1e9e", "\u0130"
REPL_POOL = ["", "!", "x" * 15, "y" * 16, "z" * 17, "<" + "r" * 298 + ">"]      # lengths 0, 1, 15, 16, 17, 300


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def geometry():
    return am.api.substitute_geometry()


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


class Batch:
    def __init__(self, hays):
        self.s = am.api._Slices(hays)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(am.api.libam().am_batch_upload(self.s.arr, self.s.n, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        am.api.libam().am_batch_destroy(self.h)


def take(b):
    """(offsets, texts) of a batch handle through the accessors; the handle is destroyed."""
    try:
        return am.api.batch_to_bytes(b)
    finally:
        am.api.libam().am_batch_destroy(b)


def with_offsets(texts):
    texts = [_b(t) for t in texts]
    return np.cumsum([0] + [len(t) for t in texts]).astype(np.uint64), texts


def same(got, exp, what):
    assert got[0].tolist() == exp[0].tolist(), (what, "offsets", got[0].tolist()[:8], exp[0].tolist()[:8])
    for i, (g, e) in enumerate(zip(got[1], exp[1])):
        if g != e:
            k = next((j for j in range(min(len(g), len(e))) if g[j] != e[j]), min(len(g), len(e)))
            raise AssertionError((what, "haystack", i, "byte", k, g[max(0, k - 8):k + 24], e[max(0, k - 8):k + 24]))
    assert len(got[1]) == len(exp[1]), what


class Subst:
    """An automaton on a route, its oracle twin, its span table and its replacements: handle v stands for by_handle[v] and is replaced by repls[v]."""

    def __init__(self, needles, repls, route=0, values=None, by_handle=None, n=None):
        self.by_handle = list(needles) if by_handle is None else by_handle
        self.n = n
        self.a = am.Automaton(needles, values)
        self.a.set_kernel(route)
        self.o = oracle.Machine(needles, values)
        self.lengths = tuple(x[:len(self.by_handle)] for x in am.api.needle_lengths(self.by_handle))
        self.t = am.SpanTable(self.a, n, lengths=self.lengths)
        self.repls = [_b(x) for x in repls][:self.t.n_needles]
        self.r = am.SubstTable(self.t, self.repls)

    def expected(self, case, hays):
        return with_offsets(sref.substitute(self.o, case, self.by_handle, hays, self.repls, self.n))

    def one_shot(self, case, hays):
        s = am.api._Slices(hays)
        b = C.c_void_p()
        am.api.check(am.api.libam().am_substitute(self.r.handle, case, s.arr, s.n, C.byref(b)))
        return take(b)

    def check(self, case, hays, exp=None, mirror=True):
        """am_substitute == am_substitute_batch == am_batch_substitute over am_spans_batch's result == the host mirror == the definition; returns the expectation."""
        exp = self.expected(case, hays) if exp is None else with_offsets(exp)
        same(self.one_shot(case, hays), exp, ("am_substitute", case))
        with Batch(hays) as b:
            same(take(self.r.substitute_batch(case, b, raw=True)), exp, ("am_substitute_batch", case))
            x = self.t.spans_batch(case, b, ref.LEFTMOST_LONGEST, raw=True)
            try:
                same(take(self.r.splice(b, x, raw=True)), exp, ("am_batch_substitute", case))
            finally:
                am.api.libam().am_spans_free(x)
        if mirror:
            got = self.a.substitute_host_mirror(case, hays, self.repls, n_values=self.t.n_needles, lengths=self.lengths)
            same(with_offsets(got), exp, ("host mirror", case))
        return exp


# ---- 1. the fragment pool

@pytest.mark.parametrize("limit", [-1, 1])
@pytest.mark.parametrize("seed", range(2))
def test_fragment_pool(route, seed, limit):
    """The pool of the span tests with replacements of length 0, 1, 15, 16, 17 and 300; AM_SPANS_CHAIN_LIMIT = 1 sends every chain of three to the doubling rounds."""
    am.debug_set("AM_SPANS_CHAIN_LIMIT", limit)
    rng = random.Random(7300 + seed)
    for i in range(8):
        needles, hays = helpers.fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]               # a needle listed twice, with a replacement of its own: the smaller handle's is used
        if i % 5 == 2 and "" not in needles:
            needles = needles + [""]                       # the empty needle inserts nothing
        if "" in needles and route == ROUTES["table_walk"]:
            continue                                       # the empty needle: no DFA section
        repls = [REPL_POOL[(v + i) % len(REPL_POOL)] + str(v) * (v % 2) for v in range(len(needles))]
        d = Subst(needles, repls, route)
        for case in (0, 1):
            exp = d.check(case, hays)
            if case == 0:
                assert exp[1] == sref.regex_substitute(needles, hays, repls)
        lowered = [oracle.lower_utf8(x).decode() for x in needles]
        if lowered != needles:
            Subst(lowered, repls, route).check(1, hays)


# ---- 2. piece ends at every destination residue

@pytest.mark.parametrize("repl", ["<>", "", "=" * 33])
def test_piece_ends_at_every_destination_residue(repl):
    G, T = geometry()
    hays = ["x" * n + "|" + "y" * m for n in range(2 * G + 2) for m in range(G + 2)]      # neighbouring haystacks share store groups
    d = Subst(["|"], [repl])
    exp = d.check(0, hays, mirror=False)
    assert exp[1][5] == _b(repl) + b"y" * 5
    ends = set(int(x) % G for x in exp[0])
    assert ends == set(range(G)) and int(exp[0][-1]) > 2 * T


# ---- 3. sources at every alignment

def test_sources_at_every_alignment():
    """Gaps and replacements that start at each source offset mod 16, the last replacement of the pool and the last gap of the batch among them: reads stay inside
    the padding."""
    G, _ = geometry()
    needles = ["<%02d>" % i for i in range(40)]
    repls = [chr(65 + i % 26) * (1 + (i * 3) % 19) for i in range(40)]
    starts = np.cumsum([0] + [len(r) for r in repls])[:-1]
    assert set(int(s) % 16 for s in starts) == set(range(16))
    rng = random.Random(3)
    hays, gap_residues, at = [], set(), 0
    for h in range(6):
        parts = []
        for k in range(40):
            gap = "g" * rng.randint(1, 19)
            gap_residues.add((at + sum(map(len, parts))) % 16)
            parts += [gap, needles[(k * 7 + h) % 40]]
        parts.append("t" * (h + 1))                                       # ... and the batch ends with a gap
        hays.append("".join(parts))
        at += len(hays[-1])
    hays.append("tail" + needles[39] + "z" * 3)                           # the last replacement of the pool; the last gap of the batch is 3 bytes before the end of the text
    assert gap_residues == set(range(16))
    d = Subst(needles, repls)
    d.check(0, hays)
    d.check(0, [hays[-1][:-3]])                                           # the batch ends with the pool's last replacement


# ---- 4. tile seams

def test_pieces_that_start_just_before_a_tile_seam():
    G, T = geometry()
    d = Subst(["|"], ["<=>"])
    for seam in (T, 2 * T):
        hays = ["x" * a + "|" + "y" * 50 for a in range(seam - G - 3, seam + 1)]      # the replacement starts at a, the gap after it at a + 3: both within G bytes before the seam
        for h in hays:
            d.check(0, [h], mirror=False)
        d.check(0, hays, mirror=False)


def test_pieces_longer_than_three_tiles_and_a_tile_of_one_byte_pieces():
    G, T = geometry()
    long = 3 * T + 5
    d = Subst(["|", "#"], ["R" * long, ""])
    d.check(0, ["ab|cd", "q" * long + "|" + "w" * long + "#", "|" * 3], mirror=False)
    d = Subst(["a", "b"], ["A", "B"])
    exp = d.check(0, ["x" + "ab" * T, "ab" * (T // 2) + "a"], mirror=False)          # every piece is one byte: T of them in a tile, and T + 1 piece ends
    assert exp[1][0] == b"x" + b"AB" * T


# ---- 5. zero-length runs and empty shapes

def test_zero_length_runs():
    d = Subst(["ab"], [""])
    exp = d.check(0, ["x", "ab" * 5000, "y", "ab" * 3 + "c" + "ab" * 700, ""])
    assert exp[1] == [b"x", b"", b"y", b"c", b""]
    d = Subst(["a"], [""])
    exp = d.check(0, ["ba", "a" * 70000, "ab", "a" * 17], mirror=False)
    assert exp[0].tolist() == [0, 1, 1, 2, 2]


def test_nothing_to_do():
    G, T = geometry()
    d = Subst(["needle", "other"], ["X", "Y"])
    hays = ["no match here " * 700, "", "x" * (T + 3), "needl"]
    exp = d.check(0, hays)                                                # no match at all: identical bytes and offsets
    assert exp[1] == [_b(h) for h in hays]
    for case in (0, 1):
        offs, texts = d.one_shot(case, [])                                # n_hay == 0
        assert offs.tolist() == [0] and texts == []
        exp = d.check(case, ["", "", ""])                                 # empty haystacks only
        assert exp[0].tolist() == [0, 0, 0, 0]
    with Batch([]) as b:
        offs, texts = take(d.r.substitute_batch(0, b, raw=True))
        assert offs.tolist() == [0] and texts == []
    d = Subst(["needle", "other"], [], n=0)                               # n_needles == 0: every handle is skipped
    exp = d.check(0, ["a needle and another", ""])
    assert exp[1] == [b"a needle and another", b""]


def test_ends(route):
    d = Subst(["ab", "abc"], ["<1>", ""], route)
    exp = d.check(0, ["abxx", "xxab", "ab", "abc", "xabcab", "abab", "b"])
    assert exp[1] == [b"<1>xx", b"xx<1>", b"<1>", b"", b"x<1>", b"<1><1>", b"b"]
    d.check(1, ["ABxx", "xxaB", "Ab", "aBC", "xabCAB", "b"])


# ---- 6. IgnoreCase: the bytes removed are the span's own

def test_ignore_case_widths(route):
    d = Subst(["k", "i"], ["K!", "[i]"], route)
    text = "kK" + KELVIN + "-" + DOTTED_I + "iI" + KELVIN + KELVIN + DOTTED_I
    exp = d.check(1, [text, KELVIN, DOTTED_I + "x", text[::-1]])
    assert exp[1][1] == b"K!" and exp[1][0].startswith(b"K!K!K!-")
    d.check(0, [text, KELVIN])
    long_needle = "kåßx" * 75                                   # 300 code points, 450 bytes; its upper-case form is 750 bytes
    upper = (KELVIN + ANGSTROM + SHARP_S + "X") * 75
    d = Subst([long_needle, "ßx", "x"], ["<long>", "", "x" * 20], route)
    hays = ["ab" + upper + long_needle + "k", upper[:-1], "x" + upper]
    exp = d.check(1, hays)
    assert exp[1][0] == b"ab<long><long>k"


# ---- 7. one chain through everything

def test_one_long_chain(route):
    d = Subst(["aa"], ["b"], route)
    text = b"a" * 100001
    want = [b"b" * 50000 + b"a"]
    for case in (0, 1):
        d.check(case, [text], exp=want, mirror=(case == 0))
    lib = am.api.libam()
    with Batch([text]) as b:
        out, sp = C.c_void_p(), C.c_void_p()
        am.api.check(lib.am_substitute_batch(d.r.handle, 0, b, C.byref(out), C.byref(sp)))
        try:
            assert lib.am_spans_rounds(sp) > 0 and lib.am_spans_size(sp) == 50000
            offs, spans = am.api.spans_to_numpy(sp)                       # the spans come in SOURCE coordinates
            assert spans["start"].tolist()[:3] == [0, 2, 4] and int(spans["start"][-1]) == 99998
        finally:
            lib.am_spans_free(sp)
        same(take(out), with_offsets(want), "spans_out")


# ---- 8. the output exceeds 2^32 bytes, the input does not

def test_output_beyond_four_gib():
    """`a` -> 64 bytes over 2^26 + 3 a's and "za": offsets [0, 2^32 + 192, 2^32 + 257].  No full readback: the bytes around 2^32 and the end through am_batch_read_text,
    the rest through am_count_batch of "y" on the result (every replacement ends in one y)."""
    import torch
    n_a = 2 ** 26 + 3
    repl = b"x" * 63 + b"y"
    dev = torch.device("cuda:0")
    text = torch.full((n_a + 2 + 30,), ord("a"), dtype=torch.uint8, device=dev)
    text[n_a] = ord("z")
    text[n_a + 2:] = 0
    offs = torch.tensor([0, n_a, n_a + 2], dtype=torch.int64, device=dev)
    d = Subst(["a"], [repl])
    lib = am.api.libam()
    b, out = C.c_void_p(), C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), 2, n_a + 2, C.byref(b)))
    try:
        am.api.check(lib.am_substitute_batch(d.r.handle, 0, b, C.byref(out), None))
        assert am.api.batch_offsets(out).tolist() == [0, 2 ** 32 + 192, 2 ** 32 + 257]
        assert lib.am_batch_total_bytes(out) == 2 ** 32 + 257 and lib.am_batch_haystacks(out) == 2
        got = am.api.batch_read_text(out, 2 ** 32 - 64, 64 + 257)
        assert got == repl * 4 + b"z" + repl, got[-80:]
        assert am.api.batch_read_text(out, 0, 130) == (repl * 3)[:130]
        y = am.Automaton(["y"])
        counts, tot = np.zeros(2, np.uint64), C.c_uint64(0)
        am.api.check(lib.am_count_batch(y.device, 0, out, counts.ctypes.data, C.byref(tot)))
        assert counts.tolist() == [n_a, 1] and tot.value == n_a + 1
        buf = np.zeros(1, np.uint8)
        assert lib.am_batch_read_text(out, 2 ** 32 + 257, 1, buf.ctypes.data) == am.AM_ERR_INVALID
    finally:
        if out.value:
            lib.am_batch_destroy(out)
        lib.am_batch_destroy(b)
        lib.am_release_device_memory()


# ---- 9. the result is a working batch

def test_the_result_feeds_the_next_device_stage(route):
    rng = random.Random(99)
    words = ["tshirt", "shirt", "shirts", "hi", "his", "irt", "k", "kk"]
    repls = ["TEE", "<shirt>", "", "hello there, ", "k", "shirt", "kk", "tshirts"]
    hays = [" ".join(rng.choice(words + ["x", "Shirt", KELVIN]) for _ in range(rng.randint(0, 40))) for _ in range(200)]
    d = Subst(words, repls, route)
    second = Subst(["shirt", "k", "TEE", "there"], ["S", "", "tee" * 7, "x"], route)
    lib = am.api.libam()
    for case in (0, 1):
        exp = d.expected(case, hays)
        with Batch(hays) as b:
            nb = d.r.substitute_batch(case, b, raw=True)
            try:
                counts, flags = np.zeros(len(hays), np.uint64), np.zeros(len(hays), np.uint8)
                am.api.check(lib.am_count_batch(second.a.device, case, nb, counts.ctypes.data, None))
                am.api.check(lib.am_contains_any_batch(second.a.device, case, nb, flags.ctypes.data))
                want = [len(second.o.run_list(case, t)[0]) for t in exp[1]]
                assert counts.tolist() == want and flags.tolist() == [int(w > 0) for w in want] and sum(want) > 100
                twice = with_offsets(sref.substitute(second.o, case, second.by_handle, exp[1], second.repls))
                same(take(second.r.substitute_batch(case, nb, raw=True)), twice, ("twice", case))
            finally:
                lib.am_batch_destroy(nb)


def test_two_runs_give_identical_bytes():
    rng = random.Random(5)
    needles = ["ab", "abc", "b", "ca", "a"]
    repls = ["1", "", "three", "4" * 20, "a"]
    hays = ["".join(rng.choice("abc ") for _ in range(rng.randint(0, 9000))) for _ in range(30)]
    d = Subst(needles, repls)
    for case in (0, 1):
        first, again = d.one_shot(case, hays), d.one_shot(case, hays)
        same(again, first, "again")
        same(first, d.expected(case, hays), "definition")
    assert d.one_shot(0, hays)[1] == sref.regex_substitute(needles, hays, repls)


# ---- 10. the accessors give back what went up

def test_accessors_return_what_was_uploaded():
    rng = random.Random(12)
    lib = am.api.libam()
    small = ["", "abc", KELVIN * 5, "", "x" * 100]                        # one buffer [offsets | text], a single copy
    large = [bytes(rng.getrandbits(8) for _ in range(1000)) * k for k in (700, 1, 0, 4300)]      # 5 MB: beyond the single-copy path
    for hays in (small, large, []):
        exp = with_offsets(hays)
        with Batch(hays) as b:
            assert lib.am_batch_haystacks(b) == len(hays) and lib.am_batch_total_bytes(b) == int(exp[0][-1])
            same(am.api.batch_to_bytes(b), exp, "accessors")
            assert lib.am_batch_device_offsets(b) and (lib.am_batch_device_text(b) or not hays)
            if hays:
                whole = b"".join(exp[1])
                for first, n in ((0, 1), (len(whole) - 1, 1), (3, len(whole) - 3), (len(whole), 0)):
                    assert am.api.batch_read_text(b, first, n) == whole[first:first + n]
                x = C.c_void_p()                                          # the device pointers describe the batch: borrowed, it reads the same
                am.api.check(lib.am_batch_from_device(lib.am_batch_device_text(b), lib.am_batch_device_offsets(b), len(hays), len(whole), C.byref(x)))
                try:
                    same(am.api.batch_to_bytes(x), exp, "borrowed")
                finally:
                    lib.am_batch_destroy(x)

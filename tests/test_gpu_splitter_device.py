"""Splitter on the device (am_split / am_split_batch / am_batch_from_fragments, csrc/am_split.hip) against the reference's fold.  Expected values are a Python
stepAccum / finalizeAccum (Splitter.hs:141-170) over oracle.Machine([sep]).run_list and oracle.skip_code_points_backwards, or literals; never another path of the library."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def fold(o, sep, ic, text):
    """splitReverse / splitReverseIgnoreCase (Splitter.hs:100-121) in forward order, as (start, len) pairs."""
    text = _b(text)
    pos, _ = o.run_list(1 if ic else 0, text)
    sep_bytes, sep_cps = len(_b(sep)), len(sep)
    out, frag_start = [], 0                                # zeroAccum :150-152
    for p in pos.tolist():
        sep_start = oracle.skip_code_points_backwards(text, p - 1, sep_cps - 1) if ic else p - sep_bytes
        if sep_start >= frag_start:                        # stepAccum :158-170
            out.append((frag_start, sep_start - frag_start))
            frag_start = p
    out.append((frag_start, len(text) - frag_start))       # finalizeAccum :141-147
    return out


def expected(sep, ic, hays):
    o = oracle.Machine([sep])
    return [fold(o, sep, ic, h) for h in hays]


class Batch:
    def __init__(self, hays):
        self.s = am.api._Slices(hays)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(am.api.libam().am_batch_upload(self.s.arr, self.s.n, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        am.api.libam().am_batch_destroy(self.h)


def per_haystack(offs, frags):
    return [[(int(s), int(n)) for s, n in frags[int(offs[i]):int(offs[i + 1])].tolist()] for i in range(len(offs) - 1)]


def check_offsets(offs, frags, hays, sep, ic):
    assert offs[0] == 0 and offs[-1] == len(frags) and (np.diff(offs.astype(np.int64)) >= 1).all()
    if not ic:
        for i, h in enumerate(hays):
            part = frags[int(offs[i]):int(offs[i + 1])]
            assert int(part["len"].sum()) + (len(part) - 1) * len(_b(sep)) == len(_b(h)), i


def check_split(sep, hays, ic, kernel=0, strings=True, exp=None):
    """am_split == am_split_batch == Python split_batch_device == the fold."""
    lib = am.api.libam()
    exp = expected(sep, ic, hays) if exp is None else exp
    sp = am.Splitter(sep)
    sp.set_kernel(kernel)
    s = am.api._Slices(hays)
    f = C.c_void_p()
    am.api.check(lib.am_split(sp.device, 1 if ic else 0, s.arr, s.n, C.byref(f)))
    try:
        assert lib.am_fragments_haystacks(f) == len(hays)
        offs, frags = am.api.fragments_to_numpy(f)
    finally:
        lib.am_fragments_free(f)
    assert per_haystack(offs, frags) == exp, ("am_split", sep, ic, kernel)
    check_offsets(offs, frags, hays, sep, ic)
    with Batch(hays) as b:
        offs_b, frags_b = sp.fragments_batch(b, ic)
    assert np.array_equal(offs_b, offs) and np.array_equal(frags_b, frags), ("am_split_batch", sep, ic, kernel)
    if strings:
        bs = [_b(h) for h in hays]
        assert sp.split_batch_device(hays, ic) == [[h[a:a + n] for a, n in e] for h, e in zip(bs, exp)], ("split_batch_device", sep, ic, kernel)
    return exp


def literal_rows():
    """tests/golden/splitter_literal_answers.json: the fold's rules as literal answers, in the row shape of the reference's golden rows."""
    import json
    import os
    from tests.conftest import ROOT
    with open(os.path.join(ROOT, "tests", "golden", "splitter_literal_answers.json")) as f:
        return json.load(f)["splitter"]


def test_golden_rows_and_literals(golden, route):
    rows = literal_rows()
    assert len(rows) == 4
    for row in golden["splitter"] + rows:
        exp = check_split(row["sep"], [row["haystack"]], row["ignore_case"], route)
        h = _b(row["haystack"])
        assert [h[a:a + n].decode("utf-8") for a, n in exp[0]] == row["expected"], row["src"]
    assert am.Splitter("aa").split_batch_device(["aaaXaa"]) == [[b"", b"aX", b""]]
    assert am.Splitter(",").split_batch_device(["a,b,,c", "", ","]) == [[b"a", b"b", b"", b"c"], [b""], [b"", b""]]
    check_split(",", ["a,b,,c", "", ","], False, route)
    check_split("aa", ["aaaXaa"], False, route)
    check_split(",", [], False, route)


def test_an_image_handle_is_refused():
    a = am.Automaton(["ab"])
    img = am.ImageAutomaton(a.image_bytes(0))
    h = C.c_void_p()
    assert am.api.libam().am_splitter_create(img.device, 2, 2, C.byref(h)) == am.AM_ERR_UNSUPPORTED and not h.value


CHAIN_LENGTHS = list(range(10)) + [63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 200001]


@pytest.mark.parametrize("limit", [1, -1])
def test_one_chain_through_everything(route, limit):
    """"aa" over a run of a's: every match overlaps the one before it, so the whole text is one chain.  n // 2 empty fragments, then "a" * (n % 2).
    AM_SPLIT_CHAIN_LIMIT = 1: the head's lane looks at one record, so every chain of three records and more (n >= 4) is finished by the doubling rounds."""
    am.debug_set("AM_SPLIT_CHAIN_LIMIT", limit)
    hays = ["a" * n for n in CHAIN_LENGTHS]
    exp = [[(2 * k, 0) for k in range(n // 2)] + [(n - n % 2, n % 2)] for n in CHAIN_LENGTHS]
    check_split("aa", hays, False, route, strings=False, exp=exp)
    rounds = am.api.libam().am_debug_split_rounds()
    assert 1 <= rounds <= 18, rounds                       # 100 000 kept records in one chain: at most ceil(log2) = 17 rounds of doubling and one that marks nothing (marks seen within a round only save rounds)
    # the long haystack alone, as strings
    got = am.Splitter("aa").split_batch_device(["a" * 2001])[0]
    assert got == [b""] * 1000 + [b"a"]


@pytest.mark.parametrize("seed", range(4))
def test_chains_with_varying_gaps(route, seed):
    """"aabaa" overlaps itself with periods 3 and 4: next[] skips one or two records, chains end and begin all over random {a, b} text."""
    rng = random.Random(4400 + seed)
    hays = ["".join(rng.choice("ab") for _ in range(n)) for n in (4096, 70000)]
    hays.append("aabaab" * 300 + "b" + "aabaaba" * 300)   # long chains with both periods
    exp = expected("aabaa", False, hays)
    assert any(len(e) > 100 for e in exp)
    for limit in (1, 3, -1):
        am.debug_set("AM_SPLIT_CHAIN_LIMIT", limit)
        check_split("aabaa", hays, False, route, strings=(limit == -1), exp=exp)


def test_chains_end_at_a_haystack_boundary(route):
    """"aa" over 9, 2 and 11 a's with the head's lane looking at one record: chains of three records and more end where a haystack ends, and the next haystack's
    first records start below the ends before them -- the search for next[] must not leave its haystack.  Over runs of a's alone every haystack keeps its even
    starts, so a jump that strays into the next haystack lands on a record that is kept anyway; with a "b" in front of the last run its kept starts are the odd
    ones, and a stray jump marks a record the fold drops."""
    am.debug_set("AM_SPLIT_CHAIN_LIMIT", 1)
    try:
        exp = check_split("aa", ["a" * 9, "a" * 2, "a" * 11], False, route)
        assert am.api.libam().am_debug_split_rounds() >= 1      # (the doubling rounds ran)
        odd = check_split("aa", ["a" * 9, "a" * 2, "b" + "a" * 11], False, route)
    finally:
        am.debug_set("AM_SPLIT_CHAIN_LIMIT", -1)
    assert exp == [[(0, 0), (2, 0), (4, 0), (6, 0), (8, 1)], [(0, 0), (2, 0)], [(0, 0), (2, 0), (4, 0), (6, 0), (8, 0), (10, 1)]]
    assert odd == exp[:2] + [[(0, 1), (3, 0), (5, 0), (7, 0), (9, 0), (11, 1)]]


def test_ignore_case_matches_of_other_byte_lengths(route):
    # "k" matches U+212A KELVIN SIGN (three bytes)
    hays = ["aKbKKc", "K", "kKKk", "x" * 100 + "K" + "y" * 29 + "K"]
    exp = check_split("k", hays, True, route)
    assert exp[0] == [(0, 1), (4, 1), (8, 0), (11, 1)]
    # "ßß": ß is two bytes, U+1E9E three; the start of a match comes from the backward walk, inside chains of overlapping matches
    rng = random.Random(77)
    hays = ["".join(rng.choice("ßẞx") if rng.random() < 0.9 else "x" for _ in range(n)) for n in (0, 1, 2, 3, 50, 3000, 30000)]
    hays.append("ẞ" * 1001)
    for limit in (1, -1):
        am.debug_set("AM_SPLIT_CHAIN_LIMIT", limit)
        exp = check_split("ßß", hays, True, route)
    assert exp[-1] == [(6 * k, 0) for k in range(500)] + [(3000, 3)]


def test_haystack_boundaries(route):
    # the first record of a haystack is a head whatever the previous haystack's positions were
    rng = random.Random(5)
    hays = ["a" * rng.randint(0, 5) for _ in range(1000)]
    for limit in (1, -1):
        am.debug_set("AM_SPLIT_CHAIN_LIMIT", limit)
        check_split("aa", hays, False, route)
    # a comma every 1-3 bytes over 70 000 bytes; cut into haystacks whose record ranges straddle the 256-record tiles of the kernels
    text = "".join("x" * rng.randint(0, 2) + "," for _ in range(35000))[:70000]
    cuts = [0, 1, 300, 301, 1111, 1112, 9000, 33333, 65536, 69999, 70000]
    hays = [text[cuts[i]:cuts[i + 1]] for i in range(len(cuts) - 1)]
    exp = check_split(",", hays, False, route)
    assert sum(len(e) for e in exp) > 30000
    check_split(",", [text], False, route)


@functools.lru_cache(maxsize=None)
def document():
    """A document of lines (some empty, one very long, the last without a newline at its end) and the dictionary its lines are searched with."""
    rng = random.Random(31)
    words = ["tshirt", "shirts", "shorts", "Klaas", "kaas", "x", "appel"]
    lines = []
    for i in range(3000):
        n = rng.choice((0, 0, 1, 2, 3, 5, 15, 16, 17, 31, 33, 80))
        lines.append(" ".join(rng.choice(words + ["abc", "de", "f"]) for _ in range(n))[:rng.randint(0, 120)])
    lines[1500] = "kaas " * 5000
    lines.append("the last line ends with the batch: shorts")
    return "\n".join(lines), lines, words


def check_lines_batch(sp, b, lines, words):
    lib = am.api.libam()
    nb, offs = sp.lines_batch(b)
    try:
        assert offs.tolist() == [0, len(lines)]
        assert lib.am_batch_total_bytes(nb) == sum(len(_b(x)) for x in lines)
        # per-line counts and flags equal the oracle on Python-split lines
        a, o = am.Automaton(words), oracle.Machine(words)
        for case in (0, 1):
            counts, flags = np.zeros(len(lines), np.uint64), np.zeros(len(lines), np.uint8)
            am.api.check(lib.am_count_batch(a.device, case, nb, counts.ctypes.data, None))
            am.api.check(lib.am_contains_any_batch(a.device, case, nb, flags.ctypes.data))
            exp = [o.count_matches(case, x) for x in lines]
            assert counts.tolist() == exp and flags.tolist() == [int(e > 0) for e in exp], case
        # every byte of every line: an automaton of all 128 single-byte needles reports each position with the byte that stands there
        ascii_a = am.Automaton([chr(c) for c in range(128)])
        m = C.c_void_p()
        am.api.check(lib.am_run_batch(ascii_a.device, 0, nb, C.byref(m)))
        try:
            recs = am.api.matches_to_numpy(m)
        finally:
            lib.am_matches_free(m)
        voff, vals = ascii_a.values_off(), ascii_a.values()
        byte_of = vals[voff[recs["state"]]]
        assert (np.diff(voff)[recs["state"]] == 1).all()
        got = [bytearray(len(_b(x))) for x in lines]
        assert len(recs) == sum(len(g) for g in got)
        start = np.zeros(len(lines) + 1, np.int64)
        start[1:] = np.cumsum([len(g) for g in got])
        flat = np.zeros(int(start[-1]), np.uint8)
        flat[start[recs["haystack"]] + recs["end_pos"].astype(np.int64) - 1] = byte_of
        assert flat.tobytes() == b"".join(_b(x) for x in lines)
    finally:
        lib.am_batch_destroy(nb)


def test_batch_from_fragments():
    doc, lines, words = document()
    sp = am.Splitter("\n")
    with Batch([doc]) as b:
        check_lines_batch(sp, b, lines, words)
    # several documents, the fragments of the later ones at every source alignment; empty documents among them
    docs = ["", "ab\ncde\n\nf", "", "x" * 15 + "\n" + "y" * 16 + "\n" + "z" * 17, "\n", "kaas"]
    exp_lines = [x for d in docs for x in d.split("\n")]
    lib = am.api.libam()
    with Batch(docs) as b:
        nb, offs = sp.lines_batch(b)
        try:
            assert offs.tolist() == [0, 1, 5, 6, 9, 11, 12]
            counts = np.zeros(len(exp_lines), np.uint64)
            a = am.Automaton(["a", "x", "y", "z", "cd"])
            am.api.check(lib.am_count_batch(a.device, 0, nb, counts.ctypes.data, None))
            o = oracle.Machine(["a", "x", "y", "z", "cd"])
            assert counts.tolist() == [o.count_matches(0, x) for x in exp_lines]
        finally:
            lib.am_batch_destroy(nb)
    # no haystack at all: an empty batch
    with Batch([]) as b:
        nb, offs = sp.lines_batch(b)
        assert offs.tolist() == [0] and lib.am_batch_total_bytes(nb) == 0
        lib.am_batch_destroy(nb)


def test_batch_from_fragments_of_a_borrowed_batch():
    import torch
    doc, lines, words = document()
    raw = _b(doc)
    dev = torch.device("cuda:0")
    text = torch.zeros((len(raw) + 15) // 16 * 16, dtype=torch.uint8, device=dev)
    text[:len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    offs = torch.tensor([0, len(raw)], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib = am.api.libam()
    b = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), 1, len(raw), C.byref(b)))
    try:
        check_lines_batch(am.Splitter("\n"), b, lines, words)
    finally:
        lib.am_batch_destroy(b)

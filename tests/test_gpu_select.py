"""Select on the device (am_select_* / am_batch_from_selection, csrc/am_select.hip) against the definition.  Every check compares the indices, the new offsets, every
byte of the new text and the zero padding up to round_up(total, 16) with what tests/select_reference.py says -- built over the oracle, Python slices or literals --
never with another path of the library.  Shapes sit on the real seams: the gather's tile and the exclusive sums' block (am_select_geometry)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, select_reference as sel, words_reference as wref

pytestmark = pytest.mark.gpu

ROUTES = {"default": 0, "suffix_filter": 2, "table_walk": 3}
KELVIN, SHARP_S, SMALL_SHARP_S = "\u212a", "\u1e9e", "\u00df"


@pytest.fixture(params=sorted(ROUTES))
def route(request):
    if request.param == "table_walk":
        am.debug_set("AM_DFA", 1)                          # (read when an image is flattened: every automaton whose table fits gets a DFA section)
    yield ROUTES[request.param]
    am.debug_set("AM_DFA", -1)


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def lib():
    return am.api.libam()


class Batch:
    def __init__(self, hays):
        self.s = am.api._Slices(hays)
        self.h = C.c_void_p()

    def __enter__(self):
        am.api.check(lib().am_batch_upload(self.s.arr, self.s.n, C.byref(self.h)))
        return self.h

    def __exit__(self, *exc):
        lib().am_batch_destroy(self.h)


def read_batch(nb):
    """(offsets, text) of a batch handle; the text is read to round_up(total, 16) -- through a borrowed batch of one haystack over the same memory -- and the bytes
    beyond total must be zero."""
    import torch
    offs = am.api.batch_offsets(nb)
    total = int(offs[-1])
    assert lib().am_batch_total_bytes(nb) == total and lib().am_batch_haystacks(nb) == len(offs) - 1
    padded = (total + 15) // 16 * 16
    if padded == 0:
        return offs, b""
    text_ptr = lib().am_batch_device_text(nb)
    assert text_ptr and text_ptr % 16 == 0
    o = torch.tensor([0, padded], dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    x = C.c_void_p()
    am.api.check(lib().am_batch_from_device(text_ptr, o.data_ptr(), 1, padded, C.byref(x)))
    try:
        whole = am.api.batch_read_text(x, 0, padded)
    finally:
        lib().am_batch_destroy(x)
    assert whole[total:] == bytes(padded - total), ("padding", whole[total:])
    return offs, whole[:total]


def check_selection(src, s, idx, offs, text, what=None):
    """The selection and the batch made from it: indices, counts, offsets, every byte, the padding."""
    idx = np.asarray(idx, np.int64)
    got = s.indices
    assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), idx), (what, got[:16].tolist(), idx[:16].tolist())
    assert s.size == len(idx) and s.total_bytes == int(offs[-1]) and s.source_haystacks == lib().am_batch_haystacks(src), what
    assert bool(lib().am_selection_device_indices(s.handle)) == (len(idx) > 0)
    nb = s.batch(src)
    try:
        got_offs, got_text = read_batch(nb)
    finally:
        lib().am_batch_destroy(nb)
    assert np.array_equal(got_offs.astype(np.int64), np.asarray(offs, np.int64)), (what, "offsets")
    if got_text != text:
        k = next((j for j in range(min(len(got_text), len(text))) if got_text[j] != text[j]), min(len(got_text), len(text)))
        raise AssertionError((what, "byte", k, got_text[max(0, k - 8):k + 24], text[max(0, k - 8):k + 24]))


def check_texts(src, s, hays, idx, what=None):
    """... where the expectation is a list of kept indices over Python texts."""
    texts = [_b(hays[i]) for i in idx]
    check_selection(src, s, idx, sel.offsets(texts), b"".join(texts), what)


# ---- 1. compaction shapes, through am_select_flags (no scan)

ONE_LAUNCH = 1 << 16                                       # csrc/am_select.cpp kOneLaunchSums: n + 1 entries up to here take the single-launch sums
SHAPE_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, "block - 1", "block", "block + 1", "2 * block + 1", ONE_LAUNCH - 2, ONE_LAUNCH - 1, ONE_LAUNCH]


def shape_size(n):
    """A haystack count of the list above; `block` = the haystacks one workgroup of the exclusive sums handles (am_select_geometry)."""
    _, block = am.api.select_geometry()
    return n if isinstance(n, int) else {"block - 1": block - 1, "block": block, "block + 1": block + 1, "2 * block + 1": 2 * block + 1}[n]


def flag_patterns(n):
    rng = np.random.default_rng(1000 + n)
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[:1] = True
    last[n - 1:] = True
    out = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "first": first, "last": last, "even": np.arange(n) % 2 == 0, "odd": np.arange(n) % 2 == 1}
    for d in (0.1, 0.5, 0.9):
        out["random %.1f" % d] = rng.random(n) < d
    return out


@pytest.mark.parametrize("n", SHAPE_SIZES)
def test_compaction_shapes(n):
    """Lengths cycle through 0 .. 49: every source and destination residue modulo 16 and modulo 4, empty haystacks kept and dropped at run starts, run ends and alone."""
    n = shape_size(n)
    lens = np.arange(n, dtype=np.int64) % 50
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    text = np.random.default_rng(n).integers(1, 256, size=max(int(offs[-1]), 1), dtype=np.uint8)[:int(offs[-1])]      # no zero byte: padding cannot pass for text
    text = np.ascontiguousarray(text)
    with Batch([(text, int(offs[i]), int(lens[i])) for i in range(n)]) as b:
        for name, flags in flag_patterns(n).items():
            for invert in (False, True):
                keep = flags != invert
                new_offs = np.zeros(int(keep.sum()) + 1, np.int64)
                new_offs[1:] = np.cumsum(lens[keep])
                exp = text[np.repeat(keep, lens)].tobytes()
                s = am.api.select_flags(b, flags.astype(np.uint8) * 7, invert)      # (non-zero = true)
                check_selection(b, s, np.flatnonzero(keep), new_offs, exp, (n, name, invert))
                if keep.all():
                    assert exp == text.tobytes()           # one run: a straight copy


# ---- 2. tile seams

def test_tile_seams():
    T, _ = am.api.select_geometry()
    rng = random.Random(5)

    def hay(n):
        return bytes(rng.randint(1, 255) for _ in range(n))

    cases = [
        ([hay(3), hay(T + 17), hay(9)], [0, 1, 0]),                            # a kept haystack longer than a tile between short ones
        ([hay(3), hay(T + 17), hay(9)], [1, 0, 1]),
        ([hay(7), hay(T - 5), hay(T + 3), hay(T - 1), hay(11)], [0, 1, 1, 1, 0]),      # a run of three that spans three tiles
        ([hay(7), hay(T - 5), hay(T + 3), hay(T - 1), hay(11)], [1, 1, 0, 1, 1]),
        ([hay(5), hay(3 * T), hay(2)], [0, 1, 0]),                             # three tiles from source residue 5
        ([hay(21), hay(3 * T), hay(2)], [0, 1, 1]),
    ]
    for d in (-1, 0, 1):                                                       # a kept total of exactly one tile, one less, one more
        cases.append(([hay(3), hay(100), hay(5), hay(T - 100 + d), hay(1)], [0, 1, 0, 1, 0]))
        cases.append(([hay(13), hay(T + d)], [0, 1]))
    for hays, flags in cases:
        with Batch(hays) as b:
            for invert in (False, True):
                idx = [i for i, f in enumerate(flags) if bool(f) != invert]
                check_texts(b, am.api.select_flags(b, flags, invert), hays, idx, ([len(h) for h in hays], flags, invert))


# ---- 3. predicates against the definition

def pool_case(seed, n_hay=300, n_needles=None, max_frags=12, alphabet=None):
    """Needles and haystacks from a shared fragment pool (helpers.fragment_case's recipe with a batch of a few hundred haystacks, some empty)."""
    rng = random.Random(seed)
    alphabet = helpers.ALPHABETS[seed % len(helpers.ALPHABETS)] if alphabet is None else alphabet
    frags = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(3, 8))]
    needles = ["".join(rng.choice(frags) for _ in range(rng.randint(1, 3))) for _ in range(n_needles if n_needles is not None else rng.randint(1, 12))]
    hays = ["".join(rng.choice(frags) for _ in range(rng.randint(0, max_frags))) for _ in range(n_hay)]
    for _ in range(6):                                     # haystacks that hold every needle, so that containsAll is true somewhere
        hays[rng.randrange(n_hay)] = "".join(rng.sample(needles, len(needles)))
    for k in range(0, n_hay, 37):
        hays[k] = ""
    return needles, hays


def lowered(needles):
    return [oracle.lower_utf8(x).decode() for x in needles]


def select_any(a, case, invert, b):
    return am.api._select(lambda out: lib().am_select_any_batch(a.device, case, int(invert), b, out))


@pytest.mark.parametrize("seed", range(4))
def test_select_any_is_contains_any(route, seed):
    needles, hays = pool_case(seed)
    for case in (0, 1):
        ns = lowered(needles) if case else needles
        a = am.Automaton(ns)
        a.set_kernel(route)
        p = sel.pred_any(ns, case)
        with Batch(hays) as b:
            for invert in (False, True):
                idx, _ = sel.keep(p, invert, hays)
                check_texts(b, select_any(a, case, invert, b), hays, idx, ("any", case, invert))
        # the one-shot form: the same indices
        s = am.api._Slices(hays)
        one = am.api._select(lambda out: lib().am_select_any(a.device, case, 0, s.arr, s.n, out))
        assert one.indices.tolist() == sel.keep(p, False, hays)[0] and one.source_haystacks == len(hays)


@pytest.mark.parametrize("no_ids_scan", [0, 1])
@pytest.mark.parametrize("n_needles", [1, 3, 40])
def test_select_all_is_contains_all(route, n_needles, no_ids_scan):
    """40 needles cross a word of the bitmap rows; AM_NO_IDS_SCAN sends containsAll through the fold over the records."""
    needles, hays = pool_case(70 + n_needles, n_needles=n_needles, alphabet="abAB12" if n_needles == 40 else None)
    am.debug_set("AM_NO_IDS_SCAN", no_ids_scan)
    try:
        for case in (0, 1):
            ns = lowered(needles) if case else needles
            a = am.Automaton(ns)
            a.set_kernel(route)
            t = am.api.ValuesTable(a)
            p = sel.pred_all(ns, case)
            with Batch(hays) as b:
                for invert in (False, True):
                    idx, _ = sel.keep(p, invert, hays)
                    if case == 0 and not invert:
                        assert 0 < len(idx) < len(hays)
                    check_texts(b, t.select_all_batch(case, b, invert), hays, idx, ("all", n_needles, case, invert))
            assert t.select_all_texts(case, hays).indices.tolist() == sel.keep(p, False, hays)[0]
    finally:
        am.debug_set("AM_NO_IDS_SCAN", -1)


@pytest.mark.parametrize("no_ids_scan", [0, 1])
def test_select_all_quirks(no_ids_scan):
    """Zero needles: every haystack is true.  [""]: never contained (AhoCorasickSpec.hs:196-200)."""
    hays = ["abc", "", "b"]
    am.debug_set("AM_NO_IDS_SCAN", no_ids_scan)
    try:
        for needles in ([], [""]):
            t = am.api.ValuesTable(am.Automaton(needles))
            with Batch(hays) as b:
                for case in (0, 1):
                    for invert in (False, True):
                        idx, _ = sel.keep(sel.pred_all(needles, case), invert, hays)
                        assert idx == ([0, 1, 2] if (needles == []) != invert else [])
                        check_texts(b, t.select_all_batch(case, b, invert), hays, idx, (needles, case, invert))
    finally:
        am.debug_set("AM_NO_IDS_SCAN", -1)


@pytest.mark.parametrize("route", [ROUTES["default"], ROUTES["suffix_filter"]])      # (the empty needle: no DFA section, no table walk)
def test_select_any_with_the_empty_needle(route):
    """An automaton that holds the empty needle beside others takes the dense route."""
    needles, hays = pool_case(11)
    needles = needles + [""]
    a = am.Automaton(needles)
    a.set_kernel(route)
    with Batch(hays) as b:
        for case in (0, 1):
            for invert in (False, True):
                idx, _ = sel.keep(sel.pred_any(needles, case), invert, hays)
                check_texts(b, select_any(a, case, invert, b), hays, idx, ("dense", case, invert))
    only = am.Automaton([""])                               # no transition at all: nothing is reported
    with Batch(hays[:5]) as b:
        check_texts(b, select_any(only, 0, False, b), hays[:5], [])
        check_texts(b, select_any(only, 0, True, b), hays[:5], [0, 1, 2, 3, 4])


def check_spans(needles, hays, case, cls, route=0, n=None):
    a = am.Automaton(needles)
    a.set_kernel(route)
    t = am.api.SpanTable(a, n, word_bytes=None if cls is None else sorted(cls))
    p = sel.pred_spans(needles, case, cls, n)
    out = []
    with Batch(hays) as b:
        for invert in (False, True):
            idx, _ = sel.keep(p, invert, hays)
            check_texts(b, t.select_batch(case, b, invert), hays, idx, ("spans", needles[:4], case, invert))
            out.append(idx)
    return out[0]


@pytest.mark.parametrize("seed", range(3))
def test_select_spans_is_a_non_empty_row(route, seed):
    needles, hays = pool_case(30 + seed)
    for case in (0, 1):
        ns = lowered(needles) if case else needles
        check_spans(ns, hays, case, None, route)                               # a plain table: every span is a row
        check_spans(ns, hays, case, wref.DEFAULT_CLASS, route)
        check_spans(ns, hays, case, wref.LOWER_CLASS, route)                   # a custom class
        if len(ns) > 1:
            check_spans(ns, hays, case, None, route, n=len(ns) - 1)            # the last handle is beyond the table


def test_select_spans_whole_words(route):
    hays = ["the", "he said", "(he)", "she", "he", "", "ache he", "hehe", "x he", "the\nhe"]
    assert check_spans(["he"], hays, 0, wref.DEFAULT_CLASS, route) == [1, 2, 4, 6, 8, 9]
    assert check_spans(["he"], hays, 0, None, route) == [0, 1, 2, 3, 4, 6, 7, 8, 9]
    # a match that touches the first or the last byte of its haystack: the neighbour is never a byte of the haystack beside it
    hays = ["ab", "ab", "xab", "abx", "ab ab", "a", "b"]
    assert check_spans(["ab"], hays, 0, wref.DEFAULT_CLASS, route) == [0, 1, 4]
    # IgnoreCase: code points whose lower case has another byte length, next to a word boundary
    hays = [KELVIN, "a " + KELVIN, KELVIN + "b", "k", "(K)", SHARP_S, "x" + SHARP_S, SHARP_S + " x", SMALL_SHARP_S + ".", "ok"]
    assert check_spans(["k", SMALL_SHARP_S], hays, 1, wref.DEFAULT_CLASS, route) == [0, 1, 3, 4, 5, 7, 8]
    assert check_spans(["k", SMALL_SHARP_S], hays, 1, None, route) == list(range(10))


def test_select_spans_with_a_zero_length_span():
    """A needle of length 0 gives an empty span, which still counts as a span (a table of one handle: the empty needle alone); whole-word: only where both
    neighbours are no word bytes."""
    hays = ["A1", "A", "Ab", "xA", "", "b", "A1x", "bA1"]
    idx = check_spans(["", "A1"], hays, 0, None, n=1)
    assert 0 < len(idx) < len(hays)
    check_spans(["", "A1"], hays, 0, wref.LOWER_CLASS, n=1)
    check_spans(["", "A1"], hays, 0, wref.DEFAULT_CLASS)


def test_select_spans_in_groups_of_bounded_record_memory():
    """AM_HIST_RECORDS_MIB = 1: 64 Ki records at a time, so a batch with more than 192 Ki values goes through in four groups or more, each with a text of its own."""
    rng = random.Random(77)
    hays = ["".join(rng.choice("abab ") for _ in range(rng.randint(0, 2400))) for _ in range(300)]
    hays[17], hays[140], hays[299] = "", "  ", "ccc"
    needles = ["a", "b", "ab"]
    o = oracle.Machine(needles)
    assert sum(o.count_matches(0, h) for h in hays) * 16 > 3 << 20
    am.debug_set("AM_HIST_RECORDS_MIB", 1)
    try:
        check_spans(needles, hays, 0, wref.DEFAULT_CLASS)
        check_spans(needles, hays, 1, None)
    finally:
        am.debug_set("AM_HIST_RECORDS_MIB", -1)


# ---- 4. composition

@functools.lru_cache(maxsize=None)
def document():
    rng = random.Random(31)
    words = ["tshirt", "shirts", "shorts", "Klaas", "kaas", "x", "appel"]
    lines = []
    for _ in range(800):
        n = rng.choice((0, 0, 1, 2, 3, 5, 15, 16, 17, 31, 33, 80))
        lines.append(" ".join(rng.choice(words + ["abc", "de", "f"]) for _ in range(n))[:rng.randint(0, 120)])
    lines[400] = "kaas " * 3000
    lines.append("the last line ends with the batch: shorts")
    return "\n".join(lines), lines, words


def check_scans_of(nb, texts, words):
    """am_count_batch and am_run_batch over a produced batch equal the oracle on the Python texts."""
    a, o = am.Automaton(words), oracle.Machine(words)
    for case in (0, 1):
        counts = np.zeros(max(len(texts), 1), np.uint64)
        am.api.check(lib().am_count_batch(a.device, case, nb, counts.ctypes.data, None))
        assert counts[:len(texts)].tolist() == [o.count_matches(case, x) for x in texts], case
        m = C.c_void_p()
        am.api.check(lib().am_run_batch(a.device, case, nb, C.byref(m)))
        try:
            recs = am.api.matches_to_numpy(m)
        finally:
            lib().am_matches_free(m)
        got = helpers.expand_records(a.values_off(), a.values(), recs["haystack"], recs["state"], recs["end_pos"])
        assert got == helpers.oracle_triples(o, case, texts), case


def test_document_to_lines_to_selected_lines():
    doc, lines, words = document()
    sp = am.Splitter("\n")
    first, second = ["kaas", "shorts"], ["shirts", "x"]
    a1, a2 = am.Automaton(first), am.Automaton(second)
    with Batch([doc]) as b:
        lb, _ = sp.lines_batch(b)
        try:
            idx1, kept1 = sel.keep(sel.pred_any(first, 0), False, lines)
            assert 0 < len(idx1) < len(lines)
            s1 = select_any(a1, 0, False, lb)
            check_texts(lb, s1, lines, idx1)
            nb = s1.batch(lb)
            try:
                check_scans_of(nb, kept1, words)
                # a selection of a selection composes through the two index arrays
                idx2, _ = sel.keep(sel.pred_any(second, 1), True, kept1)
                s2 = select_any(a2, 1, True, nb)
                check_texts(nb, s2, kept1, idx2)
                through = s1.indices[s2.indices]
                assert through.tolist() == [i for i, x in enumerate(lines) if sel.pred_any(first, 0)(_b(x)) and not sel.pred_any(second, 1)(_b(x))]
                # nothing kept: a batch of 0 haystacks and 0 bytes that every entry point accepts
                none = am.api.select_flags(nb, np.zeros(len(kept1), np.uint8))
                eb = none.batch(nb)
                try:
                    assert lib().am_batch_haystacks(eb) == 0 and lib().am_batch_total_bytes(eb) == 0 and am.api.batch_offsets(eb).tolist() == [0]
                    check_scans_of(eb, [], words)
                    flags = np.zeros(1, np.uint8)
                    am.api.check(lib().am_contains_any_batch(a1.device, 0, eb, flags.ctypes.data))
                    again = select_any(a1, 0, True, eb)
                    assert again.size == 0 and again.indices.tolist() == [] and again.source_haystacks == 0
                    eb2 = again.batch(eb)
                    assert lib().am_batch_haystacks(eb2) == 0
                    lib().am_batch_destroy(eb2)
                finally:
                    lib().am_batch_destroy(eb)
            finally:
                lib().am_batch_destroy(nb)
        finally:
            lib().am_batch_destroy(lb)


def test_a_source_batch_made_by_substitute():
    _, lines, words = document()
    lines = lines[:300]
    repls = ["T", "", "pants and more pants", "K", "cheese", "yy", "apple"]
    a = am.Automaton(words)
    r = am.api.SubstTable(am.api.SpanTable(a), repls)
    from tests import substitute_reference as sref
    rewritten = sref.substitute(oracle.Machine(words), 0, words, lines, repls)
    with Batch(lines) as b:
        sb = r.substitute_batch(0, b, raw=True)
        try:
            needles = ["cheese", "pants"]
            idx, kept = sel.keep(sel.pred_any(needles, 0), False, rewritten)
            assert 0 < len(idx) < len(lines)
            s = select_any(am.Automaton(needles), 0, False, sb)
            check_texts(sb, s, rewritten, idx)
            nb = s.batch(sb)
            try:
                check_scans_of(nb, kept, ["pants", "apple", "T"])
            finally:
                lib().am_batch_destroy(nb)
        finally:
            lib().am_batch_destroy(sb)


# ---- 5. beyond 2^32

def test_positions_beyond_4_gib():
    """A borrowed batch over 4 GiB + 2 MiB of zeros: a few hundred short haystacks planted around offset 2^32 and at the very end, the rest in a handful of huge ones."""
    import torch
    total = (4 << 30) + (2 << 20)
    edge = 1 << 32
    dev = torch.device("cuda:0")
    text = torch.zeros(total, dtype=torch.uint8, device=dev)
    rng = random.Random(9)
    planted = [bytes(rng.choice(b"needl eNEDL-") for _ in range(rng.randint(0, 40))) for _ in range(300)]
    planted[7], planted[120], planted[299] = b"a needle", b"needle", b"the last needle"
    mid, tail = planted[:200], planted[200:]
    mid_at = edge - sum(len(x) for x in mid[:100]) - 3      # the hundredth planted haystack straddles 2^32 or ends 3 bytes before it
    tail_at = total - sum(len(x) for x in tail)
    cuts = [0, mid_at // 3, mid_at // 2, mid_at]
    for x in mid:
        cuts.append(cuts[-1] + len(x))
    cuts.append(tail_at)
    for x in tail:
        cuts.append(cuts[-1] + len(x))
    assert cuts[-1] == total and cuts[3 + 100] <= edge < cuts[3 + 200] and all(a <= z for a, z in zip(cuts, cuts[1:]))
    hays_at = {3 + i: x for i, x in enumerate(mid)}
    hays_at.update({3 + 200 + 1 + i: x for i, x in enumerate(tail)})
    n = len(cuts) - 1
    for at, blob in ((mid_at, b"".join(mid)), (tail_at, b"".join(tail))):
        text[at:at + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    offs = torch.tensor(cuts, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    b = C.c_void_p()
    am.api.check(lib().am_batch_from_device(text.data_ptr(), offs.data_ptr(), n, total, C.byref(b)))
    try:
        def expect(idx):
            texts = [hays_at[i] for i in idx]
            return sel.offsets(texts), b"".join(texts)

        planted_idx = sorted(hays_at)
        for name, idx in (("both sides and one run across 2^32", planted_idx), ("alternate", planted_idx[::2]), ("across the edge only", planted_idx[90:110]),
                          ("the very end", planted_idx[-1:])):
            flags = np.zeros(n, np.uint8)
            flags[idx] = 1
            check_selection(b, am.api.select_flags(b, flags), idx, *expect(idx), what=name)
        idx = [i for i in planted_idx if b"needle" in hays_at[i]]
        assert {3 + 7, 3 + 120, n - 1} <= set(idx)
        check_selection(b, select_any(am.Automaton(["needle"]), 0, False, b), idx, *expect(idx), what="any")
    finally:
        lib().am_batch_destroy(b)
    del text


# ---- 6. errors, lifetimes

def test_the_selection_belongs_to_its_batch():
    out = C.c_void_p(1)
    with Batch(["ab", "c", "abc"]) as b, Batch(["ab", "c"]) as fewer, Batch(["ab", "c", "abcd"]) as longer, Batch(["abc", "", "abc"]) as same_shape:
        s = am.api.select_flags(b, [1, 0, 1])
        for other in (fewer, longer):
            assert lib().am_batch_from_selection(other, s.handle, C.byref(out)) == am.AM_ERR_INVALID and not out.value
            assert b"haystack count and size" in lib().am_last_error()
            out.value = 1
        out.value = None
        am.api.check(lib().am_batch_from_selection(same_shape, s.handle, C.byref(out)))      # (the same count and total: the am_batch_from_fragments rule)
        lib().am_batch_destroy(out)
        check_texts(b, s, ["ab", "c", "abc"], [0, 2])
    # free and destroy in either order
    bh = Batch(["ab", "c", "abc"])
    b = bh.__enter__()
    s = am.api.select_flags(b, [0, 1, 1])
    nb = s.batch(b)
    bh.__exit__()
    assert s.indices.tolist() == [1, 2]                    # the source batch is gone: the selection and the new batch stand alone
    del s
    assert am.api.batch_to_bytes(nb)[1] == [b"c", b"abc"]
    lib().am_batch_destroy(nb)
    bh = Batch(["ab", "c"])
    b = bh.__enter__()
    s = am.api.select_flags(b, [1, 1])
    h = s.handle
    s._h = None
    lib().am_selection_free(h)
    bh.__exit__()


def test_the_launches_have_names():
    needles, hays = pool_case(3)
    a = am.Automaton(needles)
    t = am.api.SpanTable(a)
    am.api.check(lib().am_profile_reset())
    am.api.check(lib().am_profile_enable(1))
    try:
        with Batch(hays) as b:
            s = t.select_batch(0, b)
            lib().am_batch_destroy(s.batch(b))
    finally:
        am.api.check(lib().am_profile_enable(0))
    for k in (b"select_plan", b"select_emit", b"select_gather", b"hay_flags_spans"):
        ms, n = C.c_double(0), C.c_uint64(0)
        am.api.check(lib().am_profile_read(k, C.byref(ms), C.byref(n)))
        assert n.value == 1, k

"""The definition of per-needle exact case (include/am.h "exact case") in Python: spans_reference.all_spans over the oracle's fold steps, filtered by the exact rule --
plain slicing and == --, then by the whole-word rule where a class is given, THEN spans_reference.leftmost_longest; substitute, counts and scores on top.  What the
exact-case tests expect -- never another path of the library."""
import random

from tests import spans_reference as ref
from tests import substitute_reference as sref
from tests import words_reference as wref

ALL, LEFTMOST_LONGEST = ref.ALL, ref.LEFTMOST_LONGEST
KELVIN, A_RING, ANGSTROM, DOTTED_I = "\u212a", "\u00c5", "\u212b", "\u0130"
ALPHABET = ["a", "A", "b", "B", "k", "K", KELVIN, A_RING, ANGSTROM, DOTTED_I, " "]


def _b(t):
    return t.encode("utf-8") if isinstance(t, str) else bytes(t)


def spellings(exact):
    """The spellings as bytes / None per handle."""
    return [None if x is None else _b(x) for x in exact]


def exact_case(text, start, n, spelling):
    """exact[v] is absent, or len == |exact[v]| and hay[start, start + len) == exact[v]."""
    return spelling is None or (n == len(spelling) and text[start:start + n] == spelling)


def all_spans(machine, case, needles, text, exact, cls=None, n=None):
    text, ex = _b(text), spellings(exact)
    rows = [s for s in ref.all_spans(machine, case, needles, text, n) if exact_case(text, s[0], s[1], ex[s[2]])]
    return rows if cls is None else [s for s in rows if wref.whole_word(text, s[0], s[1], cls)]


def spans(machine, case, mode, needles, hays, exact, cls=None, n=None):
    """Per haystack, the list of (start, len, handle): filter (exact, then whole words), then select."""
    rows = [all_spans(machine, case, needles, h, exact, cls, n) for h in hays]
    return [ref.leftmost_longest(r) for r in rows] if mode == LEFTMOST_LONGEST else rows


def select_then_filter(machine, case, needles, hays, exact, n=None):
    """The WRONG order -- the plain leftmost-longest selection filtered afterwards -- for tests that show the two differ."""
    ex = spellings(exact)
    out = []
    for h in hays:
        t = _b(h)
        out.append([s for s in ref.leftmost_longest(ref.all_spans(machine, case, needles, t, n)) if exact_case(t, s[0], s[1], ex[s[2]])])
    return out


def substitute(machine, case, needles, hays, replacements, exact, cls=None, n=None):
    rows = spans(machine, case, LEFTMOST_LONGEST, needles, hays, exact, cls, n)
    return [sref.splice(h, r, replacements) for h, r in zip(hays, rows)]


def highlight(machine, case, needles, hays, before, after, exact, cls=None):
    """Every selected span wrapped, the text keeping its own spelling."""
    out = []
    for h, row in zip(hays, spans(machine, case, LEFTMOST_LONGEST, needles, hays, exact, cls)):
        t, parts, cursor = _b(h), [], 0
        for s, k, _ in row:
            parts += [t[cursor:s], _b(before), t[s:s + k], _b(after)]
            cursor = s + k
        out.append(b"".join(parts) + t[cursor:])
    return out


def counts(machine, case, needles, hays, exact, cls=None, n=None):
    n = len(needles) if n is None else n
    out = [0] * n
    for row in spans(machine, case, ALL, needles, hays, exact, cls, n):
        for _, _, v in row:
            out[v] += 1
    return out


# ---- the worked examples of the header, under AM_IGNORE_CASE: (lower-cased needles, exact, text, {mode: rows})
EXAMPLES = [
    (["us", "apple", "nike"], ["US", "Apple", None], "us, US and NIKE's apple", {ALL: [(4, 2, 0), (11, 4, 2)], LEFTMOST_LONGEST: [(4, 2, 0), (11, 4, 2)]}),
    (["k"], ["K"], "K k " + KELVIN, {ALL: [(0, 1, 0)], LEFTMOST_LONGEST: [(0, 1, 0)]}),
    (["k"], [KELVIN], "K k " + KELVIN, {ALL: [(4, 3, 0)], LEFTMOST_LONGEST: [(4, 3, 0)]}),
    (["ab c", "ab"], ["AB C", None], "ab c", {ALL: [(0, 2, 1)], LEFTMOST_LONGEST: [(0, 2, 1)]}),
    (["us", "us"], ["US", None], "US", {ALL: [(0, 2, 1), (0, 2, 0)], LEFTMOST_LONGEST: [(0, 2, 0)]}),      # (a state's values come in list order: the later needle first)
    (["us", "us"], ["US", None], "us", {ALL: [(0, 2, 1)], LEFTMOST_LONGEST: [(0, 2, 1)]}),
]


def random_case(rng, lower, n_hay=None, share=0.5, n_needles=None):
    """1 to 6 needles (or n_needles) of 1 to 5 code points over ALPHABET, lower-cased with `lower` (what the automaton holds), a spelling for about `share` of the handles -- the needle as
    drawn, so it can be kept under AM_IGNORE_CASE, or its lower-cased form, which AM_CASE_SENSITIVE can keep too -- and texts of up to 120 bytes that quote the drawn
    needles often."""
    drawn = ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(1, 6) if n_needles is None else n_needles - 1)]
    if n_needles is not None or rng.random() < 0.3:
        drawn.append("".join(c.swapcase() if c.isascii() else c for c in drawn[0]))      # two handles of (often) one state
    needles = [lower(_b(d)).decode("utf-8") for d in drawn]
    # (n_needles given: exactly that share of the handles carries a spelling; otherwise each handle with that probability)
    spelled = set(rng.sample(range(len(drawn)), round(share * len(drawn)))) if n_needles is not None else {v for v in range(len(drawn)) if rng.random() < share}
    exact = [(d if rng.random() < 0.75 else n) if v in spelled else None for v, (d, n) in enumerate(zip(drawn, needles))]
    hays = []
    for _ in range(rng.randint(1, 3) if n_hay is None else n_hay):
        parts, size, limit = [], 0, rng.choice([0, 7, 30, 120, 120])
        while True:
            p = rng.choice(drawn + needles) if rng.random() < 0.5 else rng.choice(ALPHABET)
            if size + len(_b(p)) > limit:
                break
            parts.append(p)
            size += len(_b(p))
        hays.append("".join(parts))
    return needles, exact, hays


def seeded(seed, lower, count, **kw):
    rng = random.Random(seed)
    return [random_case(rng, lower, **kw) for _ in range(count)]

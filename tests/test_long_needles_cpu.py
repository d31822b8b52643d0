"""Needles of 17 bytes to 66 000 (tests/helpers.py: long_needle_sets, long_needle_text, long_needle_replacer_cases), held on the CPU to what they claim: the
image's host interpreter (general AC walk, suffix filter + resolve, resolve-everything, and the table walk where a DFA section exists) equals the oracle on
every set and text in both case modes, the brute-force oracle agrees on the needles of up to 2 049 bytes, every planted piece does what the generator lists it
for, and the Replacer cases end where they say after the number of passes they pin -- so a failure of tests/test_gpu_long_needles.py is the kernel's.  CPU only."""
import re

import numpy as np
import pytest

from oracle import naive, oracle
from tests import helpers
from tests.helpers import (LONG_ALPHABETS, LONG_BEYOND, LONG_FANOUTS, LONG_FORK_DEPTH, LONG_STEP_LENGTHS, ImgCheck, long_near_miss, long_needle_plan,
                           long_needle_replacer_cases, long_needle_sets, long_text_parts, sf_expand, sf_oracle_records)

SETS = long_needle_sets()
SET_CASES = [(name, case) for name in SETS for case in (0, 1)]
IDS = ["%s-%s" % (name, "IC" if case else "CS") for name, case in SET_CASES]

# (max_needle_cps of the image header; dfa_chunk and dfa_warm of the DFA section under AM_DFA = 1) per set and case mode, pinned: a change of the flattener's
# rule for either shows up here.  The GPU file reads the same table.
HEADER = {
    ("steps/ab", 0): (8193, 65536, 8192), ("steps/ab", 1): (8193, 65536, 8192),
    ("steps/abcdefgh", 0): (8193, 65536, 8192), ("steps/abcdefgh", 1): (8193, 65536, 8192),
    ("steps/abkåßi", 0): (6185, 65536, 8192), ("steps/abkåßi", 1): (6185, 65536, 13385),          # (IgnoreCase: the warm-up covers K for k, three bytes for one)
    ("steps/ak𝄞яß", 0): (4152, 65536, 8192), ("steps/ak𝄞яß", 1): (4152, 65536, 10827),
    ("beyond/ab", 0): (66000, 524288, 65999), ("beyond/ab", 1): (66000, 524288, 65999),
    ("beyond/ak𝄞яß", 0): (32951, 524288, 65999), ("beyond/ak𝄞яß", 1): (32951, 524288, 85682),
    ("forks/abcdefgh", 0): (744, 4096, 743), ("forks/abcdefgh", 1): (744, 4096, 743),
    ("forks/abkåßi", 0): (744, 4096, 1014), ("forks/abkåßi", 1): (744, 8192, 1626),
    ("forks/ak𝄞яß", 0): (744, 8192, 1542), ("forks/ak𝄞яß", 1): (744, 8192, 1956),
    ("periodic", 0): (8000, 32768, 7999), ("periodic", 1): (8000, 32768, 7999),
}


def nbytes(s):
    return len(s.encode("utf-8"))


_MACHINES, _RECORDS = {}, {}


def machine(name):
    if name not in _MACHINES:
        _MACHINES[name] = oracle.Machine(SETS[name])       # (the needles are lower case: the same machine serves both modes)
    return _MACHINES[name]


def records(name, case, part):
    """The oracle over one batch, computed once: (haystack, matchPos, value) arrays in fold order."""
    key = (name, case, part)
    if key not in _RECORDS:
        t = long_needle_plan(name, case, 0, part)
        _RECORDS[key] = sf_oracle_records(machine(name), case, t.text, t.offs)
    return _RECORDS[key]


def dfa_chunk_rule(forced, warm):
    """am_flatten.cpp:902-907, :918 restated: the header's dfa_warm is the deepest needle's bytes - 1; AM_DFA_CHUNK (2 048 when unset or out of range) is rounded up to
    16 and doubled until it holds four warm-ups, up to 1 MiB.  So a forced small unit does not stay small under a long needle: the warm-up never exceeds a
    quarter of the unit in an image the flattener made."""
    chunk = forced if 64 <= forced <= (1 << 20) else 2048
    chunk = (chunk + 15) & ~15
    while chunk < 4 * (warm + 1) and chunk < (1 << 20):
        chunk *= 2
    return chunk


@pytest.fixture(scope="module")
def chk():
    return ImgCheck()


def test_the_sets_hold_the_needles_they_are_built_for():
    """Nothing is dropped: every set has the number of needles its recipe gives, at the byte lengths it names, lower case, duplicates where promised."""
    assert sorted(SETS) == sorted(["steps/" + a for a in LONG_ALPHABETS] + ["beyond/" + LONG_ALPHABETS[0], "beyond/" + LONG_ALPHABETS[3]] +
                                  ["forks/" + a for a in LONG_ALPHABETS[1:]] + ["periodic"])
    k = len(LONG_STEP_LENGTHS)
    assert LONG_STEP_LENGTHS == (17, 20, 21, 22, 37, 38, 39, 55, 56, 57, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
    # what the slot line settles, and what one and two walk steps reach (tests/helpers.py quotes am_image.h): the pairs around each are in the list
    assert (helpers.LONG_SLOT_LINE, helpers.LONG_SLOT_LINE + helpers.LONG_STEP, helpers.LONG_SLOT_LINE + helpers.LONG_PARK_AFTER * helpers.LONG_STEP) == (21, 38, 55)
    assert all(b in LONG_STEP_LENGTHS and b + 1 in LONG_STEP_LENGTHS for b in (21, 38, 55))
    for name, ns in SETS.items():
        assert all(n and oracle.lower_utf8(n).decode("utf-8") == n for n in ns), name
        alphabet = name.partition("/")[2]
        if name.startswith("steps/"):
            assert len(ns) == 2 * k + 2
            assert [nbytes(n) for n in ns] == list(LONG_STEP_LENGTHS) * 2 + [57, 1024]
            base = ns[k - 1]
            assert all(base.endswith(n) for n in ns[:k]) and ns[2 * k] == ns[9] and ns[2 * k + 1] == ns[14]        # a chain of suffixes; two duplicates
            assert not any(base.endswith(n) for n in ns[k:2 * k])                                                   # the independent ones are no part of it
            assert set("".join(ns)) == set(alphabet)
        elif name.startswith("beyond/"):
            assert [nbytes(n) for n in ns] == [16500, 1025, 8193, 70, 66000, 1025, 8193, 70]
            for big, s1, s2, head in (ns[:4], ns[4:]):
                assert big.endswith(s1) and big.endswith(s2) and head.rstrip("a") == big[:len(head.rstrip("a"))]
            assert LONG_BEYOND == (16500, 66000) and LONG_BEYOND[0] > 16 * 1024 and LONG_BEYOND[1] > 65535 and LONG_BEYOND[1] > 64 * 1024
        elif name.startswith("forks/"):
            assert len(ns) == 2 * sum(f + 3 for f in LONG_FANOUTS)
            at = 0
            for depth in (LONG_FORK_DEPTH + 3, None):
                for f in LONG_FANOUTS:
                    forks, more = ns[at:at + f], ns[at + f:at + f + 3]
                    at += f + 3
                    stem = forks[0][1:]
                    assert all(n[1:] == stem for n in forks) and len({n.encode("utf-8")[-len(stem.encode("utf-8")) - 1] for n in forks}) == f      # f selector bytes
                    assert depth is None or len(stem) == depth
                    assert depth is not None or nbytes(stem) == 9 + nbytes(stem[:3])
                    assert [len(m) - len(forks[0]) for m in more] == [1, 17, 40] and all(any(m.endswith(n) for n in forks) for m in more)
        else:
            assert ns == ["ab" * 4000, "ab" * 12, "ba" * 30]


@pytest.mark.parametrize("name,case", SET_CASES, ids=IDS)
def test_the_host_interpreter_equals_the_oracle(chk, name, case):
    """ImgCheck.scan with which = 0 (general AC walk), 1 (filter + probe + resolve), 2 (resolve everything) over every batch of the set, and 3 (the table walk)
    over an image flattened under AM_DFA = 1; the header's max_needle_cps and the DFA section's chunk and warm-up are the pinned ones."""
    m = machine(name)
    vo, vals = m.values_off(), m.values()
    img = chk.flatten(m, case)
    cps = max(len(n) for n in SETS[name])
    assert ImgCheck.header(img)["max_needle_cps"] == cps
    chk.set("AM_DFA", 1)
    try:
        img_dfa = chk.flatten(m, case)
    finally:
        chk.set("AM_DFA", -1)
    d = ImgCheck.dfa_header(img_dfa)
    print("HEADER", repr((name, case)), (cps, d["chunk"], d["warm"]))
    assert d["off_next"] != 0, "no DFA section"
    assert (cps, d["chunk"], d["warm"]) == HEADER[(name, case)]
    assert d["chunk"] == dfa_chunk_rule(-1, d["warm"])
    for forced in (64, 2048):                      # the GPU file's "k_dfa 64" and "k_dfa 2048": the same warm-up, the unit the rule makes of the forced one
        chk.set("AM_DFA", 1)
        chk.set("AM_DFA_CHUNK", forced)
        try:
            f = ImgCheck.dfa_header(chk.flatten(m, case))
        finally:
            chk.set("AM_DFA", -1)
            chk.set("AM_DFA_CHUNK", -1)
        assert f["warm"] == d["warm"] and f["chunk"] == dfa_chunk_rule(forced, d["warm"]) >= 4 * d["warm"]
    for part in range(long_text_parts(name)):
        t = long_needle_plan(name, case, 0, part)
        exp = records(name, case, part)
        for which, image in ((0, img), (1, img), (2, img), (3, img_dfa)):
            n, recs = chk.scan(image, which, t.hays())
            assert n >= 0, (name, case, part, which)
            got = sf_expand(recs[0], recs[1], recs[2], vo, vals)
            assert all(np.array_equal(g, e) for g, e in zip(got, exp)), (name, case, part, which)


@pytest.mark.parametrize("name,case", SET_CASES, ids=IDS)
def test_the_texts_hold_what_they_list(name, case):
    """Every needle is planted whole (none dropped) and matched there; a near miss, a needle without its first code point and a needle cut over two haystacks give
    no record of that needle; the listed ends lie where they say relative to multiples of 1 024; empty haystacks, the mixed haystack and the batch limit."""
    ns = SETS[name]
    planted, matched = set(), set()
    kinds = set()
    for part in range(long_text_parts(name)):
        t = long_needle_plan(name, case, 0, part)
        hay, pos, val = records(name, case, part)
        assert len(t.text) <= helpers.LONG_BATCH_LIMIT and t.offs[-1] == len(t.text)
        text, offs = helpers.long_needle_text(name, case, 0, part)
        assert text == t.text and np.array_equal(offs, t.offs) and offs[0] == 0 and (np.diff(offs) >= 0).all()
        found = {}
        for h, p, v in zip(hay.tolist(), pos.tolist(), val.tolist()):
            found.setdefault(h, []).append((p, v))
        same = {i: [j for j, n in enumerate(ns) if n == ns[i]] for i in range(len(ns))}      # a duplicate needle is found as both
        for kind, i, h, detail in t.items:
            kinds.add(kind)
            b = t.text[t.offs[h]:t.offs[h + 1]]
            mine = [p for p, v in found.get(h, []) if i >= 0 and v in same[i]]
            if kind in ("whole", "cased", "plus one", "ends at", "starts at"):
                assert len(mine) == len(same[i]), (name, case, kind, i, h)
                if kind == "whole":
                    planted.add(i)
                    assert b == ns[i].encode("utf-8") and mine[0] == len(b)
                if kind == "cased":
                    assert oracle.lower_utf8(b) == ns[i].encode("utf-8") and mine[0] == len(b)
                if kind == "ends at":
                    assert (int(t.offs[h]) + mine[0] - detail) % 1024 == 0 and mine[0] == len(b)
                if kind == "starts at":
                    assert (int(t.offs[h]) + mine[0] - nbytes(ns[i]) + 1) % 1024 == 0
            elif kind in ("minus first", "cut", "near miss"):
                assert mine == [] or name == "periodic", (name, case, kind, i, h, detail)
                if kind == "near miss":
                    assert b.decode("utf-8") == long_near_miss(ns[i], detail) != ns[i] and len(b) == nbytes(ns[i])
            elif kind == "empty":
                assert len(b) == 0
            elif kind == "mixed":
                assert len(b) >= (96 << 10) and len(found.get(h, [])) > 20
            matched.update(v for _, v in found.get(h, []))
        cuts = [(i, h) for kind, i, h, _ in t.items if kind == "cut"]
        for (i, h), (i2, h2) in zip(cuts[::2], cuts[1::2]):                # the two halves are neighbours: the first one's tail would complete the match
            assert i == i2 and h2 == h + 1 and t.text[t.offs[h]:t.offs[h2 + 1]] == ns[i].encode("utf-8")
        assert int((np.diff(t.offs) == 0).sum()) >= 3
    assert planted == set(range(len(ns))), "a needle was dropped from the text"
    assert matched == set(range(len(ns))), "a needle is never matched"
    assert kinds >= {"whole", "minus first", "plus one", "cut", "near miss", "ends at", "starts at", "empty", "mixed"} | ({"cased"} if case else set())
    if name == "periodic":
        # "ab" * 12 minus its first code point, or cut, still ends in a shorter needle's text, but never in itself; the long one has no such excuse
        t = long_needle_plan(name, case)
        hay, pos, val = records(name, case, 0)
        for kind, i, h, detail in t.items:
            if kind in ("minus first", "cut", "near miss"):
                assert not ((hay == h) & (val == i)).any(), (kind, i, h)
        h = [h for kind, _, h, _ in t.items if kind == "periodic"][0]
        assert t.offs[h + 1] - t.offs[h] == 64 << 10
        assert int(((hay == h) & (val == 0)).sum()) == ((64 << 10) - 8000) // 2 + 1        # every second position from byte 8 000 on ends "ab" * 4000


@pytest.mark.parametrize("name", list(SETS))
def test_the_brute_force_oracle_agrees_up_to_2049_bytes(name):
    """oracle/naive.py (quadratic: up to 24 of the set's needles of up to 2 049 bytes, over planted pieces of the longest of them and the head of the mixed
    haystack) against the C oracle with the same needles."""
    ns = [n for n in SETS[name] if nbytes(n) <= 2049]
    ns = ns[::max(1, len(ns) // 24)][:23] + [max(ns, key=nbytes)]
    m = oracle.Machine(ns)
    longest = SETS[name].index(ns[-1])
    for case in (0, 1):
        t = long_needle_plan(name, case)
        hays = [t.text[t.offs[h]:t.offs[h + 1]] for kind, i, h, detail in t.items if i == longest and (kind in ("whole", "cased", "plus one") or detail in (1, 56))]
        mixed = t.hays()[-1][:3000]
        while mixed and (mixed[-1] & 0xC0) == 0x80:
            mixed = mixed[:-1]
        if mixed and mixed[-1] >= 0xC0:                        # (the code point the cut went through)
            mixed = mixed[:-1]
        hays.append(mixed)
        assert len(hays) >= 5
        for b in hays:
            pos, val = m.run_list(case, b)
            assert [(int(p), int(v)) for p, v in zip(pos, val)] == naive.all_matches(ns, b.decode("utf-8"), bool(case)), (name, case)


RP_CASES = long_needle_replacer_cases()


def test_the_replacer_limit_values_restate_the_hosts_rule():
    """am_replacer.cpp:835-838: ov = the longest needle's bytes (CaseSensitive) or 4 * code points + 4 (IgnoreCase); the one-kernel route takes the replacer while
    round_up_64(2 ov + longest replacement + 16) <= 4096."""
    def cap(ov, rl=1):
        return (2 * ov + rl + 16 + 63) // 64 * 64
    lo, hi = helpers.LONG_RP_CS_LIMIT
    assert hi == lo + 1 and cap(lo) <= 4096 < cap(hi)
    lo, hi = helpers.LONG_RP_IC_LIMIT
    assert hi == lo + 1 and cap(4 * lo + 4) <= 4096 < cap(4 * hi + 4)
    by_name = {c.name: c for c in RP_CASES}
    for name, ov, took in (("limit 2039 CS", 2039, True), ("limit 2040 CS", 2040, False), ("limit 508 IC", 2036, True), ("limit 509 IC", 2040, False)):
        c = by_name[name]
        assert c.ov == ov == helpers.reach(c.case, c.pairs) and (c.cap <= 4096) == took and c.cap == cap(ov)
        n = c.pairs[1][0]
        assert (len(n) if c.case else nbytes(n)) == int(name.split()[1])
    assert len(RP_CASES) == 2 * 12 + 2 and len(by_name) == len(RP_CASES)
    assert {len(c.pairs[1][0]) // 2 for c in RP_CASES if "+" in c.name and "upper" not in c.name} == {8, 100, 223, 224, 500, 1000, 3000}


@pytest.mark.parametrize("c", RP_CASES, ids=[c.name for c in RP_CASES])
def test_replacer_cases_end_where_they_say(c):
    """oracle.Replacer reaches the listed text -- "!" where N formed, nothing else touched -- for every document, after the pinned number of scans; a replacer
    WITHOUT the first pair leaves the documents alone (N is not there before "@" becomes "#")."""
    orc = oracle.Replacer(c.case, c.pairs)
    later = oracle.Replacer(c.case, c.pairs[1:])
    assert c.passes == len(c.pairs)
    for doc, want in zip(c.docs, c.expect):
        assert want.count(b"!") == 1 and doc.count("@") == 1
        assert orc.run(doc) == want, c
        assert later.run(doc) == doc.encode("utf-8"), c
        assert helpers.replacer_passes(c.case, c.pairs, doc) == (want, c.passes), c
    if "upper" in c.name:
        assert all(nbytes(d) > len(d) for d in c.docs) and any(ch in "".join(c.docs) for ch in "KİẞÅ")
    neighbours = helpers.ordinary_documents()
    assert max(helpers.replacer_passes(c.case, c.pairs, d)[1] for d in neighbours) <= c.passes


def test_nothing_is_skipped():
    """Neither this file nor the GPU file skips or expects a failure anywhere, and both run every set in both case modes."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    for f in ("test_long_needles_cpu.py", "test_gpu_long_needles.py"):
        with open(os.path.join(here, f)) as fh:
            src = fh.read()
        assert not re.search(r"mark\.(skip|xfail)|pytest\.(skip|xfail)\(", src), f
    from tests import test_gpu_long_needles as gpu
    assert sorted(gpu.SET_CASES) == sorted(SET_CASES) and len(SET_CASES) == 2 * len(SETS) == 20

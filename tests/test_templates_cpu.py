"""am_subst_table_create_templates and the front-end on top of it (include/am.h "substitute templates"): the definition (tests/template_reference.py) gives the header's
worked examples and equals an independent regex formulation with the template translated to \\g<0>; the host mirror's sequential splice (amh_substitute_templates_fold,
no device) equals the definition; an all-literal template set is the plain substitute; the entry point exists, is bound and checks its arguments before any device
work; the shared piece arithmetic of csrc/am_subst_tpl.h holds against the sequential definition under a sanitizer, in a stand-alone program.

No span table can be made without a device (am_needle_ids_create needs one): there the checks are seen with null handles."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import oracle
from tests import helpers, substitute_reference as sref, template_reference as tref
from tests.conftest import ROOT

M = am.MATCH
KELVIN = "\u212a"

# the header's worked examples and the identities it states: (needles, templates, text, case, expected)
TABLE = [
    (["nike"], [["<b>", M, "</b>"]], "NIKE nike", 1, b"<b>NIKE</b> <b>nike</b>"),
    (["ab"], [[M, M]], "xabx", 0, b"xababx"),
    (["a"], [[]], "banana", 0, b"bnn"),                                   # no segments: the match is deleted
    (["an", "b"], [[M], [M]], "banana", 0, b"banana"),                    # [MATCH]: the identity
    (["b", "abc", "abcd"], [["X"], ["Y"], ["Z"]], "abcd b", 0, b"Z X"),   # [literal]: the plain replacement
    (["k"], [["[", M, "]"]], "k" + KELVIN + "K.", 1, b"[k][\xe2\x84\xaa][K]."),      # the text's own spelling and width
    (["ab", "ab"], [["1", M], ["2", M]], "abab", 0, b"1ab1ab"),           # the smallest handle of equal spans
    (["", "a"], [["!", M], [M, "-"]], "banana", 0, b"ba-na-na-"),         # the empty needle inserts nothing
    (["x"], [[M, "y"]], "", 0, b""),
]
SHAPES = [lambda l: [], lambda l: [M], lambda l: [l[0]], lambda l: [l[0], M, l[1]], lambda l: [M, M], lambda l: [M, l[0], M],
          lambda l: [l[k % 2] if k % 2 == 0 else M for k in range(64)]]  # 64 segments alternating
LITS = ["", "!", "x" * 15, "y" * 16, "z" * 17, "<" + "r" * 298 + ">"]     # lengths 0, 1, 15, 16, 17, 300


def _gpu():
    import torch
    return torch.cuda.is_available()


def templates_for(n, salt):
    """One template per handle, the shapes and literal lengths taking turns."""
    return [SHAPES[(v + salt) % len(SHAPES)]([LITS[(v + salt) % len(LITS)], LITS[(v * 5 + salt + 1) % len(LITS)] + str(v)]) for v in range(n)]


def _fold(case, o, hays, lengths, templates, word_bytes=None):
    """amh_substitute_templates_fold over the oracle's fold steps."""
    triples = helpers.oracle_triples(o, case, hays)
    cols = list(zip(*triples)) if triples else ((), (), ())
    arrays = tuple(np.array(c, dtype=t) for c, t in zip(cols, (np.uint32, np.uint64, np.uint32)))
    return am.api.substitute_templates_fold_host(case, arrays, hays, lengths[0], lengths[1], templates, word_bytes)


def test_the_definition_gives_the_worked_examples():
    for needles, tpls, text, case, want in TABLE:
        assert tref.substitute(oracle.Machine(needles), case, needles, [text], tpls) == [want], (needles, text)
        if case == 0:
            assert tref.regex_substitute(needles, [text], tpls) == [want], (needles, text)
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    assert '"<b>NIKE</b> <b>nike</b>"' in doc and '"xababx"' in doc      # ... and they are the header's


def _random_template(rng, alphabet):
    return [M if rng.random() < 0.45 else "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 3))) for _ in range(rng.randint(0, 4))]


@pytest.mark.parametrize("seed", range(4))
def test_the_definition_equals_the_regex_formulation(seed):
    """600 cases: duplicate and empty needles over a three-byte alphabet, literals with a backslash among them."""
    rng = random.Random(2600 + seed)
    for _ in range(150):
        needles = ["".join(rng.choice("abc") for _ in range(rng.randint(0, 4))) for _ in range(rng.randint(1, 6))]
        tpls = [_random_template(rng, "abcXY\\&") for _ in needles]
        hays = ["".join(rng.choice("abc") for _ in range(rng.randint(0, 30))) for _ in range(3)]
        assert tref.substitute(oracle.Machine(needles), 0, needles, hays, tpls) == tref.regex_substitute(needles, hays, tpls), (needles, tpls, hays)


@pytest.mark.parametrize("seed", range(2))
def test_the_definition_equals_the_regex_formulation_ignoring_ascii_case(seed):
    """ASCII only: lower-case needles, texts in both cases; the match keeps the text's spelling."""
    rng = random.Random(2650 + seed)
    kept = 0
    for _ in range(100):
        needles = ["".join(rng.choice("abc") for _ in range(rng.randint(0, 4))) for _ in range(rng.randint(1, 6))]
        tpls = [_random_template(rng, "abcXY") for _ in needles]
        hays = ["".join(rng.choice("abcABC") for _ in range(rng.randint(0, 30))) for _ in range(3)]
        exp = tref.substitute(oracle.Machine(needles), 1, needles, hays, tpls)
        assert exp == tref.regex_substitute(needles, hays, tpls, ignore_case=True), (needles, tpls, hays)
        kept += exp != tref.substitute(oracle.Machine(needles), 1, needles, [h.lower() for h in hays], tpls)
    assert kept > 50


def test_the_host_splice_gives_the_worked_examples_without_a_device():
    for needles, tpls, text, case, want in TABLE:
        lb, lc = am.api.needle_lengths(needles)
        n = len(needles)
        assert _fold(case, oracle.Machine(needles), [text], (lb[:n], lc[:n]), tpls) == [want], (needles, text)


@pytest.mark.parametrize("seed", range(4))
def test_the_host_splice_equals_the_definition_on_the_fragment_pool(seed):
    rng = random.Random(4100 + seed)                                      # the 44 cases of tests/test_substitute_cpu.py
    for i in range(11):
        needles, hays = helpers.fragment_case(rng)
        if i % 3 == 0:
            needles = needles + [needles[0]]                              # a duplicate needle with a template of its own: the smaller handle's is used
        o = oracle.Machine(needles)
        for n in (len(needles), max(0, len(needles) - 2)):                # n below the largest handle: the last two needles are skipped
            lb, lc = am.api.needle_lengths(needles, n)
            tpls = templates_for(n, seed + i)
            for case in (0, 1):
                exp = tref.substitute(o, case, needles, hays, tpls, n)
                assert _fold(case, o, hays, (lb[:n], lc[:n]), tpls) == exp, (seed, needles, hays, n, case)
                if case == 0 and n == len(needles):
                    assert tref.regex_substitute(needles, hays, tpls) == exp, (seed, needles, hays)


@pytest.mark.parametrize("seed", range(2))
def test_all_literal_templates_are_the_plain_substitute(seed):
    rng = random.Random(4300 + seed)
    for i in range(8):
        needles, hays = helpers.fragment_case(rng)
        o = oracle.Machine(needles)
        repls = [LITS[(v + i) % len(LITS)] + str(v) * (v % 2) for v in range(len(needles))]
        lb, lc = am.api.needle_lengths(needles)
        n = len(needles)
        for case in (0, 1):
            plain = sref.substitute(o, case, needles, hays, repls)
            assert tref.substitute(o, case, needles, hays, [[r] for r in repls]) == plain
            assert tref.substitute(o, case, needles, hays, repls) == plain            # a plain replacement is the template of that literal
            assert _fold(case, o, hays, (lb[:n], lc[:n]), [[r] for r in repls]) == plain
            assert _fold(case, o, hays, (lb[:n], lc[:n]), [["", r[:1], r[1:]] for r in repls]) == plain


def test_whole_word_templates_without_a_device():
    from tests import words_reference as wref
    needles = ["he", "the"]
    tpls = [["<b>", M, "</b>"], [M]]
    lb, lc = am.api.needle_lengths(needles)
    o = oracle.Machine(needles)
    got = _fold(0, o, ["the he she"], (lb[:2], lc[:2]), tpls, word_bytes=True)
    assert got == [b"the <b>he</b> she"] == tref.substitute(o, 0, needles, ["the he she"], tpls, cls=wref.DEFAULT_CLASS)
    assert _fold(0, o, ["the he she"], (lb[:2], lc[:2]), tpls) == [b"the <b>he</b> s<b>he</b>"]


def test_header_declares_and_front_end_binds_the_entry_point():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = am.api.libam()
    n = "am_subst_table_create_templates"
    assert re.search(r"AM_API\s+[^;(]*\b%s\s*\(" % n, src)
    assert n in am.api.ABI and hasattr(lib, n)
    assert re.search(r"#define AM_SUBST_MAX_SEGMENTS 64", src) and re.search(r"#define AM_SEG_LITERAL 0", src) and re.search(r"#define AM_SEG_MATCH 1", src)
    assert (am.api.SUBST_MAX_SEGMENTS, am.api.SEG_LITERAL, am.api.SEG_MATCH) == (64, 0, 1)
    for h in ("amh_substitute_templates", "amh_substitute_templates_fold"):
        assert hasattr(am.api.libhost(), h), h
    assert len(am.api.DEBUG_ABI) == 14                     # no new am_debug_* symbol
    assert repr(am.MATCH) == "am.MATCH" and am.MATCH is am.api.MATCH
    for name in ("substitute", "highlight", "mask", "substitute_templates_host_mirror"):
        assert hasattr(am.Automaton, name), name
    assert hasattr(am.api, "substitute_templates_fold_host")
    csrc = os.path.join(ROOT, "alfred-margaret_amd", "csrc")
    shared = open(os.path.join(csrc, "am_subst_tpl.h")).read()
    assert "subst_tpl_piece" in shared and "__host__ __device__" in shared
    kernels = open(os.path.join(csrc, "am_subst.hip")).read()
    for k in ("k_subst_tpl_count", "k_subst_tpl_pieces", "k_subst_pieces", "subst_tpl_piece("):
        assert k in kernels, k
    assert "substituteTemplates" in open(os.path.join(ROOT, "alfred-margaret_amd", "host", "spans.hpp")).read()


def test_header_block_states_the_semantics():
    doc = open(os.path.join(ROOT, "include", "am.h")).read()
    part = doc[doc.index("---- substitute templates"):doc.index("am_subst_table_create_templates(const")]
    for phrase in ("T(v, m)", "AM_SEG_MATCH", "deletes the match", "identity", "OWN SPELLING", "word class", "csrc/am_subst_tpl.h", "1 + nseg", "seg_off[0] != 0",
                   "AM_SUBST_MAX_SEGMENTS", "unknown kind", "lit_off[0] != 0", "non-empty range on a MATCH segment", "2^32 bytes", "must outlive", "before any device work"):
        assert phrase in part, phrase


def test_every_argument_is_refused_before_any_device_work():
    lib = am.api.libam()
    out = C.c_void_p(1)

    def refused(rc, word):
        assert rc == am.AM_ERR_INVALID and not out.value and word in lib.am_last_error(), (rc, out.value, lib.am_last_error())
        out.value = 1

    off = np.zeros(2, np.uint64)
    assert lib.am_subst_table_create_templates(None, off.ctypes.data, None, None, None, None) == am.AM_ERR_INVALID
    refused(lib.am_subst_table_create_templates(None, off.ctypes.data, None, None, None, C.byref(out)), b"null span table or seg_off")
    with pytest.raises(am.AmError):
        am.api._pack_templates([["a", 7]], 1)              # a segment that is neither bytes, str nor am.MATCH
    with pytest.raises(am.AmError):
        am.api._pack_templates([["a"]], 2)                 # one template per handle
    if not _gpu():
        return
    a = am.Automaton(["ab", "c", "d"])
    t = am.SpanTable(a)

    def create(seg_off, kinds, lit_off, pool=b"xxxxxxxx"):
        seg_off, lit_off = np.asarray(seg_off, np.uint64), None if lit_off is None else np.asarray(lit_off, np.uint64)
        kinds = None if kinds is None else np.asarray(kinds, np.uint8)
        rc = lib.am_subst_table_create_templates(t.handle, seg_off.ctypes.data, None if kinds is None else kinds.ctypes.data,
                                                 None if lit_off is None else lit_off.ctypes.data, pool, C.byref(out))
        if rc == am.AM_OK:
            lib.am_subst_table_destroy(out)
            out.value = None
        return rc

    refused(lib.am_subst_table_create_templates(t.handle, None, None, None, None, C.byref(out)), b"null span table or seg_off")
    refused(create([1, 2, 3, 4], [0] * 4, [0] * 5), b"seg_off[0] must be 0")
    refused(create([0, 2, 1, 3], [0] * 3, [0] * 4), b"seg_off descends")
    refused(create([0, 65, 65, 65], [1] * 65, [0] * 66), b"AM_SUBST_MAX_SEGMENTS")
    refused(create([0, 1, 2, 3], None, [0] * 4), b"seg_kind or lit_off is null")
    refused(create([0, 1, 2, 3], [0] * 3, None), b"seg_kind or lit_off is null")
    refused(create([0, 1, 2, 3], [0, 2, 1], [0, 1, 1, 1]), b"unknown segment kind")
    refused(create([0, 1, 2, 3], [0, 0, 1], [1, 1, 1, 1]), b"lit_off[0] must be 0")
    refused(create([0, 1, 2, 3], [0, 0, 1], [0, 2, 1, 1]), b"lit_off descends")
    refused(create([0, 1, 2, 3], [0, 0, 1], [0, 1, 2, 3]), b"MATCH segment with literal bytes")
    refused(create([0, 1, 2, 3], [0, 0, 1], [0, 1, 1 + (1 << 32), 1 + (1 << 32)]), b"2^32 bytes")
    refused(create([0, 1, 2, 3], [0, 0, 1], [0, 1, 2, 2], pool=None), b"lit_bytes is null")
    out.value = None
    assert create([0, 0, 0, 0], None, None, pool=None) == am.AM_OK        # no segment at all needs no other array
    assert create([0, 64, 64, 65], [1] * 65, [0] * 66, pool=None) == am.AM_OK      # 64 segments, no literal byte
    assert create([0, 1, 2, 3], [0, 0, 1], [0, 1, 8, 8]) == am.AM_OK


def test_the_front_end_takes_the_old_constructor_for_plain_replacements():
    seg_off, kind, lit_off, pool = am.api._pack_templates([["<", M, ">"], "plain", []], 3)
    assert seg_off.tolist() == [0, 3, 4, 4] and kind.tolist()[:4] == [0, 1, 0, 0] and lit_off.tolist() == [0, 1, 1, 2, 7] and pool == b"<>plain"
    if not _gpu():
        a = am.Automaton(["nike"])
        for call in (lambda: a.highlight(1, ["NIKE shoe"], "<b>", "</b>"), lambda: a.mask(1, ["NIKE shoe"]), lambda: a.substitute(0, ["nike"], [[M, M]]),
                     lambda: a.substitute_templates_host_mirror(0, ["nike"], [[M, M]])):
            with pytest.raises(am.AmError) as e:
                call()
            assert e.value.code == am.AM_ERR_NO_DEVICE
        return
    t = am.SpanTable(am.Automaton(["ab", "c"]))
    assert not am.SubstTable(t, ["1", b"2"]).templates and am.SubstTable(t, ["1", [M]]).templates and am.SubstTable(t, [("1",), "2"]).templates
    assert am.Automaton(["nike"]).highlight(am.IGNORE_CASE, ["NIKE shoe"], "<b>", "</b>") == [b"<b>NIKE</b> shoe"]


@pytest.mark.parametrize("case", [0, 1])
def test_mask_is_one_fill_per_code_point(case):
    """mask's fixed replacements over the sequential splice (and, with a device, mask itself) against re.sub(lambda m: fill * len(m.group())) on str: a span has as
    many code points as its needle in both case modes.  Case 1: ASCII letters in both cases, the other code points have no case."""
    rng = random.Random(77 + case)
    needles = ["nike", "åb", "\U0001d11e", "ab\U0001f4a9c", "b", "nik"]
    order = sorted(range(len(needles)), key=lambda v: (-len(needles[v].encode()), v))
    rx = re.compile("|".join(re.escape(needles[v]) for v in order), re.I if case else 0)
    words = needles + ["x", " ", "å", "\U0001f4a9"] + (["NIKE", "Nike", "aB\U0001f4a9C", "B"] if case else [])
    hays = ["".join(rng.choice(words) for _ in range(rng.randint(0, 30))) for _ in range(40)]
    a = am.Automaton(needles)
    o = oracle.Machine(needles)
    lb, lc = am.api.needle_lengths(needles)
    for fill in ("*", "█"):
        want = [rx.sub(lambda m: fill * len(m.group()), h).encode() for h in hays]
        assert want != [h.encode() for h in hays]
        triples = helpers.oracle_triples(o, case, hays)
        arrays = tuple(np.array(c, dtype=t) for c, t in zip(zip(*triples), (np.uint32, np.uint64, np.uint32)))
        assert am.api.substitute_fold_host(case, arrays, hays, lb[:len(needles)], lc[:len(needles)], a.mask_replacements(fill)) == want
        if _gpu():
            assert a.mask(case, hays, fill) == want
    assert "code point" in am.Automaton.mask.__doc__ and "makeMatch" in am.Automaton.mask.__doc__


def test_the_shared_piece_arithmetic_holds_under_a_sanitizer(tmp_path):
    """tests/native/subst_templates_main.cpp: the piece plan of csrc/am_subst_tpl.h on the CPU, step by step as the kernels run it, against host/spans.hpp
    substituteTemplates, byte for byte; compiled with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked in statically.  A stand-alone program: no
    Python code runs under a sanitizer."""
    exe = str(tmp_path / "subst_templates")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "alfred-margaret_amd", "csrc"), "-I", os.path.join(ROOT, "alfred-margaret_amd", "host"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "subst_templates_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)      # (the runtimes are linked into the program: it starts in the environment as it is)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])

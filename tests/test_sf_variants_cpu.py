"""Which k_sf instantiation launch_sf_t (csrc/am_kernels.hip) picks, restated in Python and held to the flattener on the CPU: the needle families of tests/helpers.py
sit in the header cells they claim, every variant the rule can return is either launched by a case of tests/test_gpu_sf_variants.py or on UNREACHED below, and the
image's host interpreter agrees with the oracle on every family's text -- so a failure of the GPU file is the kernel's and not the flattener's.  CPU only."""
import itertools
import struct

import numpy as np
import pytest

from oracle import oracle
from tests import filter_keys
from tests.helpers import SF_FAMILIES, ImgCheck, sf_expand, sf_family_needles, sf_oracle_records, sf_text

LIGHT_CHUNKS = 16          # kSfLightChunks: batches of up to 16 KiB take the light configuration
MODES = ("count", "emit", "any", "ids")
FAMILIES = [f + s for f in SF_FAMILIES for s in ("", "+short")]

# family -> per case mode (CaseSensitive, IgnoreCase) the four header fields launch_sf_t reads: sf_bloom_log2_words, tier_log2_cap[3], sf_tiers & 7, sf_t4_children.
# test_header_cells holds them to the flattener; the GPU file derives the variant it expects from them.
CELLS = {
    "small": ({"lw": 11, "cap3": 11, "tiers": 0, "children": 0}, {"lw": 11, "cap3": 11, "tiers": 0, "children": 0}),
    "mid": ({"lw": 15, "cap3": 15, "tiers": 0, "children": 0}, {"lw": 15, "cap3": 15, "tiers": 0, "children": 0}),
    "large": ({"lw": 15, "cap3": 16, "tiers": 0, "children": 0}, {"lw": 15, "cap3": 16, "tiers": 0, "children": 0}),
    "dict": ({"lw": 11, "cap3": 13, "tiers": 0, "children": 5579}, {"lw": 12, "cap3": 13, "tiers": 0, "children": 7359}),
    "forked": ({"lw": 14, "cap3": 16, "tiers": 0, "children": 40000}, {"lw": 14, "cap3": 16, "tiers": 0, "children": 45823}),
}
for _f in list(CELLS):
    CELLS[_f + "+short"] = tuple(dict(c, tiers=7) for c in CELLS[_f])

# family -> what the family is there for: (ILP, LW, SHORT, CHILDREN) of the full-size count / emit launch.  The numbers of CELLS may move with a family, this may not.
PURPOSE = {"small": (1, 0, False, False), "mid": (1, 15, False, False), "large": (2, 15, False, False), "dict": (2, 0, False, True),
           "forked": (2, 0, False, True),
           "small+short": (1, 0, True, False), "mid+short": (1, 15, True, False), "large+short": (2, 15, True, False), "dict+short": (1, 0, True, False),
           "forked+short": (2, 0, True, False)}


def launch_rule(cell, ic, mode, chunks, trace=False):
    """launch_sf_t: the template arguments of the k_sf launch for an image with the header fields `cell`, a batch of `chunks` KiB chunks, under AM_SF_TRACE or not,
    as api.decode_sf_variant names them."""
    short, lw15, flag = bool(cell["tiers"] & 7), cell["lw"] == 15, mode in ("any", "ids")
    v = {"ic": bool(ic), "mode": mode, "ilp": 2, "lw": 0, "short": short, "dbg": False, "light": False, "children": False}
    if mode == "ids":
        v["light"] = chunks <= LIGHT_CHUNKS
    elif trace and not flag:
        v.update(dbg=True, lw=15 if lw15 else 0, short=short or not lw15)
    elif chunks <= LIGHT_CHUNKS:
        v["light"] = True
    elif not lw15 and cell["children"] and not short and not flag:
        v["children"] = True
    else:
        v.update(ilp=1 if cell["cap3"] <= 15 else 2, lw=15 if lw15 else 0)
    return v


def key(v):
    return tuple(sorted(v.items()))


def every_variant():
    """Every variant the rule can return, over every value of its inputs (also combinations no flattener produces: they add nothing the others do not)."""
    out = set()
    for ic, mode, tiers, lw, cap3, children, chunks, trace in itertools.product((0, 1), MODES, (0, 7), (11, 15), (15, 16), (0, 9), (LIGHT_CHUNKS, LIGHT_CHUNKS + 1), (False, True)):
        out.add(key(launch_rule({"lw": lw, "cap3": cap3, "tiers": tiers, "children": children}, ic, mode, chunks, trace)))
    return out


# Variants no input of the GPU file reaches: a suffix table of more than 2^15 buckets (tier_log2_cap[3] >= 16) behind a filter of fewer than 2^15 words, WITHOUT
# short needles.  The flattener sizes the filter by the distinct suffix keys and the table by the keys plus the child entries of heavy nodes (am_flatten.cpp), so such an
# image has child entries, and the count / emit launch of an image with child entries and no short needle is the CHILDREN instantiation.  (With a short needle, and in
# containsAny, the cell is reached: the families "forked+short" and "forked"; the natural-language dictionary does not get there with up to 200 000 words,
# profiles/r12_sf_variants.md.  The ids instantiations run <ILP 2, LW 0> for every image.)
UNREACHED = [{"ic": ic, "mode": mode, "ilp": 2, "lw": 0, "short": False, "dbg": False, "light": False, "children": False} for ic in (False, True) for mode in ("count", "emit")]


@pytest.fixture(scope="module")
def chk():
    return ImgCheck()


_MACHINES = {}


def machine(family):
    if family not in _MACHINES:
        _MACHINES[family] = oracle.Machine(sf_family_needles(family))
    return _MACHINES[family]


def cell_of(img):
    h = filter_keys.header(img)
    children, = struct.unpack_from("<I", img[:256].tobytes(), 248)          # ImageHeader::sf_t4_children
    return {"lw": h["sf_bloom_log2_words"], "cap3": h["cap3"], "tiers": h["sf_tiers"] & 7, "children": children}


@pytest.mark.parametrize("case", (0, 1))
@pytest.mark.parametrize("family", FAMILIES)
def test_header_cells_and_host_interpreter(chk, family, case):
    """The image of every family has the header fields CELLS states, they put its full-size count / emit launch into the cell the family is there for, and the image's
    host interpreter (filter + probe + resolve, and resolve-everything) finds the oracle's matches in the family's 256-KiB text."""
    m = machine(family)
    img = chk.flatten(m, case)
    cell = cell_of(img)
    assert cell == CELLS[family][case], (family, case, cell)
    v = launch_rule(cell, case, "emit", 256)
    assert (v["ilp"], v["lw"], v["short"], v["children"]) == PURPOSE[family], (family, case, v)
    if family.startswith(("dict", "forked")):          # the flag modes and the SHORT kernels ignore the child entries of these images: <ILP 1 or 2, LW 0>
        a = launch_rule(cell, case, "any", 256)
        assert cell["children"] > 0 and (a["ilp"], a["lw"], a["children"]) == (2 if family.startswith("forked") else 1, 0, False)
    text, offs = sf_text(family, case, 256 * 1024)
    hays = [text[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    exp = sf_oracle_records(m, case, text, offs)
    assert len(exp[0]) > 5000
    flags = np.zeros(len(hays), bool)
    flags[exp[0]] = True
    assert flags.any() and not flags[np.diff(offs) > 0].all() and (np.diff(offs) == 0).any()          # containsAny has a False to get wrong, and empty haystacks
    vo, vals = m.values_off(), m.values()
    for which in (1, 2):
        n, recs = chk.scan(img, which, hays)
        assert n >= 0
        got = sf_expand(recs[0], recs[1], recs[2], vo, vals)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), (family, case, which)


def test_every_variant_is_launched_by_a_gpu_case_or_listed_as_unreached():
    from tests import test_gpu_sf_variants as gpu
    claimed = {key(v) for v in gpu.claimed_variants()}
    unreached = {key(v) for v in UNREACHED}
    everything = every_variant()
    assert len(everything) == 84
    assert not claimed & unreached
    assert claimed | unreached == everything, sorted(everything ^ (claimed | unreached))
    for v in UNREACHED:                    # the list may hold nothing else
        assert v["mode"] in ("count", "emit", "any") and (v["ilp"], v["lw"]) == (2, 0) and not v["children"] and not v["dbg"] and not v["light"]


def test_variant_word_round_trip():
    """api.decode_sf_variant against the bit layout include/am_debug.h documents."""
    import alfred_margaret_amd as am
    assert am.api.decode_sf_variant(0) is None
    for k in every_variant():
        v = dict(k)
        word = 1 | v["ic"] << 1 | MODES.index(v["mode"]) << 2 | v["ilp"] << 4 | v["short"] << 6 | v["dbg"] << 7 | v["light"] << 8 | v["children"] << 9 | v["lw"] << 16
        assert am.api.decode_sf_variant(word) == v

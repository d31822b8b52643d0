"""Shared helpers for the parity tests (test infrastructure)."""
import ctypes as C
import random
import struct

import numpy as np

from oracle import oracle

ALPHABETS = ["abAB12", "яЯåÅÅ𝄞💩ßẞ", "aİkKKσΣςi", "ab"]


def fragment_case(rng, n_hay_max=5, hay_frags=40, allow_empty_needle=True):
    """tests/Data/Text/TestInstances.hs:46-93 restated: needles and haystacks from a shared fragment pool."""
    alphabet = rng.choice(ALPHABETS)
    frags = ["".join(rng.choice(alphabet) for _ in range(rng.randint(1, 5))) for _ in range(rng.randint(1, 8))]
    needles = ["".join(rng.choice(frags) for _ in range(rng.randint(1, 3))) for _ in range(rng.randint(1, 12))]
    if allow_empty_needle and rng.random() < 0.1:
        needles.append("")
    hays = ["".join(rng.choice(frags) for _ in range(rng.randint(0, hay_frags))) for _ in range(rng.randint(1, n_hay_max))]
    if rng.random() < 0.3:
        hays.insert(rng.randint(0, len(hays)), "")
    return needles, hays


def oracle_triples(machine, case, hays):
    """What the reference's fold sees: [(haystack, matchPos, value)] in fold order."""
    out = []
    for i, h in enumerate(hays):
        pos, val = machine.run_list(case, h)
        out += [(i, int(p), int(v)) for p, v in zip(pos, val)]
    return out


def expand_records(values_off, values, hay, state, end):
    out = []
    for i in range(len(hay)):
        vs = values[int(values_off[state[i]]):int(values_off[state[i] + 1])]
        out += [(int(hay[i]), int(end[i]), int(v)) for v in vs]
    return out


class ImgCheck:
    """ctypes front-end of the TEST-ONLY host interpreter of the device image (libam_imgcheck.so)."""

    def __init__(self):
        from alfred_margaret_amd import build
        self.lib = C.CDLL(build.build_imgcheck())
        self.lib.amchk_flatten.restype = C.c_longlong
        self.lib.amchk_flatten_ex.restype = C.c_longlong
        self.lib.amchk_scan.restype = C.c_longlong

    def flatten(self, m, case, lower_pairs=None):
        """m: anything with transitions()/offsets()/root_ascii()/values_off()/n_states (oracle or product machine).
        lower_pairs: the caller's lower-case table [(c, toLower c)] (am_automaton_create_ex); None = built-in."""
        tr, of, ra = m.transitions(), m.offsets(), m.root_ascii()
        vl = np.diff(m.values_off()).astype(np.uint32)
        err = C.create_string_buffer(256)
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        if lower_pairs is None:
            low = (None, None, C.c_size_t(0))
        else:
            lf = np.ascontiguousarray([a for a, _ in lower_pairs], dtype=np.uint32)
            lt = np.ascontiguousarray([b for _, b in lower_pairs], dtype=np.uint32)
            low = (P(lf), P(lt), C.c_size_t(len(lf)))
        args = (P(tr), C.c_size_t(len(tr)), P(of), C.c_size_t(m.n_states), P(ra), P(vl), case) + low
        n = self.lib.amchk_flatten_ex(*args, None, C.c_size_t(0), err, C.c_size_t(256))
        if n < 0:
            raise ValueError(err.value.decode())
        img = np.zeros(n, dtype=np.uint8)
        assert self.lib.amchk_flatten_ex(*args, P(img), C.c_size_t(n), err, C.c_size_t(256)) == n
        return img

    def scan(self, img, which, hays):
        blob, offs = oracle.pack_texts(hays)
        text = np.frombuffer(blob + b"\0", dtype=np.uint8)
        cap = max(16, len(blob) + 16)
        hay, st = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        end, vl = np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)
        P = lambda a: a.ctypes.data_as(C.c_void_p)
        n = self.lib.amchk_scan(P(img), which, P(text), P(offs), C.c_uint32(len(hays)), P(hay), P(st), P(end), P(vl), C.c_size_t(cap))
        if n < 0:
            return n, None
        return n, (hay[:n], st[:n], end[:n], vl[:n])

    def set(self, name, value):
        """A switch of csrc/am_config.h inside libam_imgcheck.so's copy of the flattener (AM_DFA, AM_DFA_CHUNK, AM_SF_NO_CHILDREN ...); -1 = unset."""
        self.lib.amchk_set.argtypes = [C.c_char_p, C.c_long]
        assert self.lib.amchk_set(name.encode(), int(value)) == 0, name

    @staticmethod
    def dfa_header(img):
        f = struct.unpack_from("<5Q2IQ4IQ2IQ", img.tobytes()[256:352])      # ImageHeader.off_dfa_next ... off_dfa_chain2
        return {"off_next": f[0], "off_out": f[1], "off_cls": f[2], "off_fail": f[3], "off_rare": f[4], "rare_log2_cap": f[5], "n_rows": f[6], "off_chain": f[7],
                "n_states": f[8], "log2_classes": f[9], "warm": f[10], "chunk": f[11], "off_hot": f[12], "hot_log2": f[13], "n_single": f[14], "off_chain2": f[15]}

    @staticmethod
    def set_dfa_chunk(img, chunk):
        img[324:328] = np.frombuffer(struct.pack("<I", chunk), dtype=np.uint8)   # ImageHeader.dfa_chunk (the host interpreter takes any value >= 1)

    @staticmethod
    def set_ac_chunk(img, chunk):
        img[36:40] = np.frombuffer(struct.pack("<I", chunk), dtype=np.uint8)   # ImageHeader.ac_chunk

    @staticmethod
    def header(img):
        f = struct.unpack_from("<4IQ4I", img.tobytes()[:40])
        return {"magic": f[0], "version": f[1], "case_mode": f[2], "total_bytes": f[4], "n_states": f[5],
                "max_needle_cps": f[6], "root_vlen": f[7], "ac_chunk": f[8]}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# A Replacer with the CALLER'S OWN priorities (include/am.h: am_replacer_create takes any distinct priorities <= 0), and the inputs that sit on
# the capacity limits of the one-kernel loop (csrc/am_rplds.hip).  tests/test_oracle_priorities.py checks on the CPU that these inputs are what
# they claim to be; tests/test_gpu_replacer_priorities.py feeds them to the kernels.

INT32_MIN = -2**31
WIDE_PRIORITIES = (INT32_MIN, INT32_MIN - 1, -2**40, -2**62)      # the edge of RpStateOne's 32-bit priority and beyond it (INT64_MIN is the fold's seed, Replacer.hs:222: never a priority)


def priority_families(rng, n):
    """{name: priorities of n payloads}: a permutation of 0 .. -(n-1); -3i-1 permuted (gaps, no zero); small ones mixed with 64-bit ones."""
    def perm():
        p = list(range(n))
        rng.shuffle(p)
        return p
    fams = {"permuted": [-i for i in perm()], "gaps": [-3 * i - 1 for i in perm()]}
    wide = [-5 * i for i in perm()]
    for k, w in zip(rng.sample(range(n), min(n, len(WIDE_PRIORITIES))), rng.sample(WIDE_PRIORITIES, len(WIDE_PRIORITIES))):
        wide[k] = w
    fams["wide"] = wide
    return fams


def sorted_by_priority(pairs, priorities):
    """The pair list that Replacer.build turns into the same replacer: runWithLimit only COMPARES priorities (Replacer.hs:236-258), so the order is all that counts."""
    return [pairs[i] for i in sorted(range(len(pairs)), key=lambda i: -priorities[i])]


def mirror_twin(pairs):
    """The same replacer as build's (priority = -index), written so that am_replacer_create does not recognise it: the list reversed, priorities -(n-1-i)."""
    n = len(pairs)
    return list(reversed(pairs)), [-(n - 1 - i) for i in range(n)]


PAYLOAD_DTYPE = np.dtype([("priority", np.int64), ("len_bytes", np.uint32), ("len_code_points", np.uint32), ("repl_off", np.uint64), ("repl_len", np.uint32), ("reserved", np.uint32)])   # am_payload


class AbiReplacer:
    """am_replacer_create called directly (ctypes), as a caller of include/am.h would: the automaton over the needles (lower-cased first under IgnoreCase,
    Replacer.hs:105-107), machineValues from the host mirror's automaton (value = needle index), the caller's am_payload[] (lengths of the ORIGINAL needle,
    :112-113) and min_priority.  priorities=None: -index, which the library recognises as Replacer.build's (the payload-implicit kernel)."""

    def __init__(self, case, pairs, priorities=None, min_priority=None, built_case=None):
        """built_case: the case sensitivity the replacer was BUILT with, where setCaseSensitivity (Replacer.hs:148-153) changed it afterwards: the needles are
        lower-cased by the built mode, scan and makeMatch run in `case`."""
        import alfred_margaret_amd as am
        self.am = am
        n = len(pairs)
        prio = [-i for i in range(n)] if priorities is None else [int(p) for p in priorities]
        if min_priority is None:
            min_priority = min(prio) if prio else 1
        orig = [p[0].encode("utf-8") if isinstance(p[0], str) else bytes(p[0]) for p in pairs]
        repl = [p[1].encode("utf-8") if isinstance(p[1], str) else bytes(p[1]) for p in pairs]
        self.automaton = am.Automaton([am.lower_utf8(b) if (case if built_case is None else built_case) else b for b in orig])      # must outlive the replacer
        self.voff = np.ascontiguousarray(self.automaton.values_off(), dtype=np.uint64)
        self.vals = np.ascontiguousarray(self.automaton.values(), dtype=np.uint32)
        pl = np.zeros(max(n, 1), PAYLOAD_DTYPE)
        off = 0
        for i in range(n):
            pl[i] = (prio[i], len(orig[i]), len(orig[i].decode("utf-8")), off, len(repl[i]), 0)
            off += len(repl[i])
        blob = b"".join(repl)
        self.payloads, self.priorities, self.min_priority = pl, prio, int(min_priority)
        h = C.c_void_p()
        vals_ptr = self.vals.ctypes.data if self.vals.size else None
        self.rc = am.libam().am_replacer_create(self.automaton.device, case, self.voff.ctypes.data, vals_ptr, pl.ctypes.data if n else None, n,
                                                blob if blob else None, len(blob), self.min_priority, C.byref(h))
        self._h = h if self.rc == 0 else None
        if self.rc != 0:
            self.error = (am.libam().am_last_error() or b"").decode("utf-8", "replace")

    def __del__(self):
        if getattr(self, "_h", None):
            self.am.libam().am_replacer_destroy(self._h)
            self._h = None

    def run(self, hays, max_len=-1):
        """am_replacer_run on slices: ([text or None per haystack], am_replaced_passes)."""
        am = self.am
        s = am.api._Slices(hays)
        res = C.c_void_p()
        am.api.check(am.libam().am_replacer_run(self._h, s.arr, s.n, 2**64 - 1 if max_len < 0 else int(max_len), C.byref(res)))
        try:
            assert int(am.libam().am_replaced_size(res)) == s.n
            out = []
            for i in range(s.n):
                p, ln = C.c_void_p(), C.c_size_t(0)
                just = am.libam().am_replaced_get(res, i, C.byref(p), C.byref(ln))
                assert just in (0, 1), just
                out.append(C.string_at(p, ln.value) if just else None)
            return out, int(am.libam().am_replaced_passes(res))
        finally:
            am.libam().am_replaced_free(res)

    def run_priority(self, hays, thresholds):
        """am_run_priority: (best priority per haystack, [(haystack, start, len, payload)])."""
        am = self.am
        s = am.api._Slices(hays)
        thr = np.ascontiguousarray(thresholds, dtype=np.int64)
        best = np.zeros(max(s.n, 1), np.int64)
        p, n = C.c_void_p(), C.c_size_t(0)
        am.api.check(am.libam().am_run_priority(self._h, s.arr, s.n, thr.ctypes.data, best.ctypes.data, C.byref(p), C.byref(n)))
        try:
            k = int(n.value)
            dt = am.api.PRIO_MATCH_DTYPE
            ms = np.frombuffer((C.c_char * (k * dt.itemsize)).from_address(p.value), dtype=dt).copy() if k else np.zeros(0, dt)
        finally:
            am.libam().am_prio_matches_free(p)
        return [int(b) for b in best[:s.n]], [(int(m["haystack"]), int(m["start"]), int(m["len"]), int(m["payload"])) for m in ms]


# ---- the limits of k_rp_lds (csrc/am_rplds.hip), one sweep per limit -------------------------------------------------------------------------
LDS_REC = 512          # kLdsRec   (am_rplds.hip:40): records of a haystack; first scan :96, list + staged new records :405, list growth :432
LDS_PC = 448           # kLdsPc    (am_rplds.hip:42): piece entries INCLUDING the sentinel (:320: np + s + 1 > kLdsPc gives up), so 447 pieces of text
LDS_WIN = 448          # kLdsWin   (am_rplds.hip:44): bytes of a re-scan window (:266)
LDS_NEW = 64           # new records of one window (:405, nf + nfb > kWave)
NEVER = ("zz", "y")    # the lowest priority of every sweep, never matches: the measured pass is not the last priority (:261, :272 edit the piece list only there)
NAMES = "abcdefghijklmnopqrstuvwxyz0123456789"


def reach(case, pairs):
    """`ov` of the one-kernel loop (am_replacer.cpp:884-885): the longest needle in bytes for CaseSensitive, 4 * code points + 4 under IgnoreCase."""
    if case:
        return 4 * max(len(n) for n, _ in pairs) + 4
    return max(len(n.encode("utf-8")) for n, _ in pairs)


class Sweep:
    """One quantity of one haystack moves across its documented limit; `fits[i]` says whether haystack i stays within the limit as csrc/am_rplds.hip states it."""

    QUANTITY = {"first-scan records": "first_scan", "list growth": "records_after", "staged records": "new_records", "pieces": "pieces", "window": "window", "new records": "new_records"}

    def __init__(self, name, case, pairs, hays, values, limit, fits):
        self.name, self.case, self.pairs, self.hays, self.values, self.limit, self.fits = name, case, pairs, hays, values, limit, fits
        self.quantity = self.QUANTITY[name.split(",")[0]]      # the key of sweep_quantities() that moves

    def __repr__(self):
        return "Sweep(%s, case=%d)" % (self.name, self.case)


def _up(case, s):
    return s.upper() if case else s


def sweep_first_scan_records(case):
    """1. 508 .. 516 match positions in the FIRST scan (:126 nr0 > kLdsRec).  The needle is eight "a"s in a run of n + 7, not "a" in a run of n: every kept match
    becomes a piece, and 508 single-byte replacements would cross the piece limit first; here a pass keeps ~64 matches."""
    pairs = [("a" * 8, "b"), NEVER]
    values = list(range(LDS_REC - 4, LDS_REC + 5))
    return Sweep("first-scan records", case, pairs, [_up(case, "a") * (n + 7) for n in values], values, LDS_REC, [n <= LDS_REC for n in values])


def sweep_growing_list(case):
    """2a. The list grows during the first pass: twenty replacements, each brings 25 match positions of the lower-priority needle (eight "q"s in a run of 32) and frees
    one slot; j + 20 records of the first scan become j + 500.  The new records are STAGED behind the list (:461 nr + nf + nfb > kLdsRec) before they move into it, so a
    step that frees `room` slots needs nr + nf <= 512 and the list can end at 512 - room = 511 at most; the growth check behind it (:432) can then never fire."""
    pairs = [("m", "q" * 32), ("q" * 8, "r"), NEVER]
    values = list(range(LDS_REC - 4, LDS_REC + 5))               # records after the first pass
    hays = [_up(case, "q" * (n - 500 + 7) + "x" * 40 + ("m" + "x" * 40) * 20) for n in values]
    return Sweep("list growth", case, pairs, hays, values, LDS_REC - 1, [n <= LDS_REC - 1 for n in values])


def sweep_staging(case):
    """2b. 490 records in the list, ONE window that brings 18 .. 26 new ones (:461): list + staged records <= 512, so 22 fit."""
    values = list(range(18, 27))
    pairs = [("m" + NAMES[i], "q" * (w + 7)) for i, w in enumerate(values)] + [("q" * 8, "r"), NEVER]
    hays = [_up(case, "q" * (489 + 7) + "x" * 40 + "m" + NAMES[i] + "x" * 40) for i, _ in enumerate(values)]
    return Sweep("staged records", case, pairs, hays, values, LDS_REC - 490, [490 + w <= LDS_REC for w in values])


def sweep_pieces(case, variant):
    """3. k non-adjacent single-byte replacements.  variant "inner": b + (ab)^k, 2k + 1 pieces; "edge": (ab)^k starts with a match, 2k pieces; "tail": (ba)^k ENDS with a
    match, 2k pieces (no tail piece behind the last replacement, has_tail :318, in a text that goes on to fill the list); "empty": the empty
    replacement leaves k + 1 pieces of text around k holes (no replacement piece, has_repl :374).  The list holds kLdsPc entries with its sentinel (:376)."""
    if variant == "empty":
        values = list(range(LDS_PC - 5, LDS_PC + 4))                # pieces
        pairs = [("a", ""), NEVER]
        hays = [_up(case, "b" + "ab" * (p - 1)) for p in values]
    else:
        ks = list(range(220, 228))
        pairs = [("a", "X"), NEVER]
        hays = [_up(case, "ba" * k if variant == "tail" else ("b" if variant == "inner" else "") + "ab" * k) for k in ks]
        values = [2 * k + (1 if variant == "inner" else 0) for k in ks]
    return Sweep("pieces, " + variant, case, pairs, hays, values, LDS_PC - 1, [p + 1 <= LDS_PC for p in values])


def sweep_window(case, variant):
    """4. One match, replacement of rl bytes: the re-scanned window is rl + 2 ov bytes ("middle"), or rl + ov where the text's start ("start") or end ("end") clips it
    (:318-322 wlen > kLdsWin).  Needles "m?" of two bytes, so ov is the same for every haystack."""
    ov = reach(case, [("mm", ""), NEVER])
    values = list(range(LDS_WIN - 8, LDS_WIN + 9))                  # window bytes
    rls = [w - (2 * ov if variant == "middle" else ov) for w in values]
    pairs = [("m" + NAMES[i], "R" * rl) for i, rl in enumerate(rls)] + [NEVER]
    pad = "x" * 600
    hays = [_up(case, (pad if variant != "start" else "") + "m" + NAMES[i] + (pad if variant != "end" else "")) for i, _ in enumerate(rls)]
    return Sweep("window, " + variant, case, pairs, hays, values, LDS_WIN, [w <= LDS_WIN for w in values])


def sweep_new_records(case, variant):
    """5. The replacement text holds m match positions of a lower-priority needle ("q").  The window is scanned 64 positions per trip from the replacement's first byte
    (:437): "one trip": m = 60 .. 64 positions in the first 64 bytes of the replacement, and 65 .. 68 that run into the second; "two trips": 40 in the first trip and
    20 .. 28 in the second (:461 nf + nfb > kWave)."""
    values = list(range(LDS_NEW - 4, LDS_NEW + 5))
    if variant == "one trip":
        repls = ["q" * m for m in values]
    else:
        repls = ["q" * 40 + "x" * 30 + "q" * (m - 40) for m in values]
    pairs = [("m" + NAMES[i], _up(case, r)) for i, r in enumerate(repls)] + [("q", "r"), NEVER]
    hays = [_up(case, "x" * 100 + "m" + NAMES[i] + "x" * 100) for i, _ in enumerate(values)]
    return Sweep("new records, " + variant, case, pairs, hays, values, LDS_NEW, [m <= LDS_NEW for m in values])


def sweep_quantities(sw, i):
    """What haystack i of a sweep does to the lists of k_rp_lds, computed with the oracle's automaton and plain Python (no kernel): the first pass is the one
    the sweeps measure.  first_scan: positions with a match (= records); pieces: entries of the piece list after the first pass; window: the longest re-scan window
    (hi - ws, am_rplds.hip:262-265); new_records: the most lower-priority match positions one window finds; records_after: the list after the first pass."""
    case, hay = sw.case, sw.hays[i].encode("utf-8")
    orig = [n.encode("utf-8") for n, _ in sw.pairs]
    repl = [r.encode("utf-8") for _, r in sw.pairs]
    m = oracle.Machine([oracle.lower_utf8(n) if case else n for n in orig])
    ov = reach(case, sw.pairs)
    pos, val = m.run_list(case, hay)
    first_scan = len(set(int(p) for p in pos))
    top = min(int(v) for v in val)
    found = []
    for p, v in zip(pos, val):
        if int(v) == top:
            p = int(p)
            st = oracle.skip_code_points_backwards(hay, p - 1, len(sw.pairs[top][0]) - 1) if case else p - len(orig[top])
            found.append((st, p - st))
    kept = []
    for st, ln in sorted(found):
        if not kept or st >= kept[-1][0] + kept[-1][1]:
            kept.append((st, ln))
    rl = len(repl[top])
    out, at, pieces = b"", 0, 0
    new_start = []
    for st, ln in kept:
        pieces += (1 if st > at else 0) + (1 if rl else 0)
        out += hay[at:st]
        new_start.append(len(out))
        out += repl[top]
        at = st + ln
    pieces += 1 if at < len(hay) or not kept else 0
    out += hay[at:]
    pos2, val2 = m.run_list(case, out)
    lower = sorted(set(int(p) for p, v in zip(pos2, val2) if int(v) > top))
    window, new_records = 0, 0
    for k in range(len(kept) - 1, -1, -1):
        ms = kept[k][0]
        newlen = len(out) - (new_start[k] - ms)                  # the text while match k is replaced: old to its left, new to its right
        hi, ws = min(ms + rl + ov, newlen), max(ms - ov, 0)
        window = max(window, hi - ws if hi > ms else 0)
        lo2, hi2 = new_start[k], new_start[k] + (hi - ms)
        new_records = max(new_records, sum(1 for p in lower if lo2 < p <= hi2))
    return {"first_scan": first_scan, "pieces": pieces, "window": window, "new_records": new_records, "records_after": len(lower), "kept": len(kept)}


def all_sweeps():
    out = []
    for case in (0, 1):
        out += [sweep_first_scan_records(case), sweep_growing_list(case), sweep_staging(case)]
        out += [sweep_pieces(case, v) for v in ("inner", "edge", "tail", "empty")]
        out += [sweep_window(case, v) for v in ("middle", "start", "end")]
        out += [sweep_new_records(case, v) for v in ("one trip", "two trips")]
    return out


def ordinary_documents(n=70, seed=3):
    """Short documents that finish in LDS under every sweep's replacer: the neighbours of section 7.  The record, piece and growth sweeps rewrite them a little
    (runs of "a" and "q", "zz"); no "m", so the long replacements of the window sweeps stay out of them and ALL of them stay within every limit."""
    rng = random.Random(seed)
    return ["".join(rng.choice(["a", "b", "x", "q", " ", "aaaaaaaa", "qqqqqqqq", "z"]) for _ in range(rng.randint(0, 40))) for _ in range(n)]


# 6. the host's route limits (am_replacer.cpp:886-887, :952)
ROUTE_REPL_LENGTHS = ((4013, 4096), (4076, 4096), (4077, 4160))      # (longest replacement, round_up_64(2 ov + rl + 16)) with ov = 2
ROUTE_MATCH_PAIRS = [("a" * 8, "b"), NEVER]
ROUTE_MATCH_COUNTS = (4095, 4096, 4097)


def route_window_pairs(rl):
    return [("m", "R" * rl), NEVER]


def route_match_document(n):
    return "a" * (n + 7)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Automata that contain the EMPTY needle (csrc/am_dense.hip k_dense): text whose code points are first code points of a needle about half of the time, haystack
# cuts that put several haystacks into one 32-byte bitmap word and multi-byte code points onto word and unit boundaries, and a plain reference of what the
# reference folds there.  tests/test_dense_units_cpu.py checks on the CPU that these are what they claim; tests/test_gpu_dense_units.py feeds them to the kernels.

DENSE_WORD = 32        # bytes of text per bitmap word of k_dense
DENSE_CHUNK = 1024     # kSfChunk: a work unit is unit_chunks of these (am.api.sf_unit_chunks)

# name -> (case, needles, [(code point, weight)]): the weights of the first code points add up to about one half, a few percent of the code points complete a needle
DENSE_SETS = {
    "sensitive": (0, ["", "ab", "b", "éa", "日本", "𝄞"],
                  [("a", 20), ("é", 10), ("日", 10), ("𝄞", 5), ("b", 3), ("x", 20), ("ü", 10), ("語", 10), ("💩", 7), ("本", 5), ("É", 3)]),
    # first code points reached through lower-casings that change the byte length: U+212A (3 bytes) -> k, İ (2) -> i, U+212B (3) -> å (2), ẞ (3) -> ß (2)
    "ignore": (1, ["", "ka", "i", "åb", "ß"],
               [("K", 8), ("K", 8), ("k", 6), ("İ", 2), ("I", 2), ("Å", 8), ("Å", 8), ("å", 4), ("ẞ", 3),
                ("a", 6), ("A", 4), ("b", 4), ("x", 17), ("Ж", 10), ("ж", 5), ("ü", 5)]),
}
DENSE_ONLY_SETS = {"empty alone": (0, [""]), "upper-case needle": (1, ["", "É"])}      # no sparse record at all; the second has sf_tiers == 0


def dense_text(rng, n_bytes, alphabet):
    """Valid UTF-8 of at most n_bytes (fewer by up to three): code points drawn from [(code point, weight)]."""
    enc = [c.encode("utf-8") for c, _ in alphabet]
    mean = sum(len(e) * w for e, (_, w) in zip(enc, alphabet)) / sum(w for _, w in alphabet)
    out = b"".join(rng.choices(enc, weights=[w for _, w in alphabet], k=int(n_bytes / mean * 1.05) + 8))
    assert len(out) >= n_bytes
    cut = n_bytes
    while (out[cut] & 0xC0) == 0x80:
        cut -= 1
    return out[:cut]


def ragged_cuts(text, rng, unit_bytes=DENSE_CHUNK, big=3 << 20):
    """Haystack offsets (np.int64, first 0, last len(text)) on code-point boundaries only, from a repeating pattern of lengths: tiny ones, 200 of 0-12 bytes, the
    sizes around 1 KiB and 64 KiB, four haystacks that END where a multi-byte code point ends a 32-byte word, two that end so on a unit's last byte, and one of
    `big` bytes.  A length that falls inside a code point is rounded down to its start."""
    t = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    n = len(t)
    multi_end = np.zeros(n + 1, dtype=bool)                      # multi_end[p]: a multi-byte code point ends with byte p - 1
    multi_end[1:n] = ((t[:n - 1] & 0xC0) == 0x80) & ((t[1:] & 0xC0) != 0x80)
    multi_end[n] = n > 0 and (t[n - 1] & 0xC0) == 0x80
    at_word = np.flatnonzero(multi_end[::DENSE_WORD]) * DENSE_WORD
    at_unit = np.flatnonzero(multi_end[::unit_bytes]) * unit_bytes
    pattern = [0, 0, 1, 2, 3, 5, 31, 32, 33, 40] + [rng.randint(0, 12) for _ in range(200)] + [1023, 1024, 1025, 65535, 65536, 65537] + [at_word] * 4 + [at_unit] * 2 + [big]
    cuts, at, k = [0], 0, 0
    while at < n:
        step = pattern[k % len(pattern)]
        k += 1
        if isinstance(step, np.ndarray):
            i = int(np.searchsorted(step, at, side="right"))
            nxt = int(step[i]) if i < len(step) else n
        else:
            nxt = min(n, at + step)
            while nxt < n and (t[nxt] & 0xC0) == 0x80:
                nxt -= 1
        cuts.append(nxt)
        at = nxt
    return np.asarray(cuts, dtype=np.int64)


def dense_reference(case, needles, text, offs):
    """What the reference folds over a batch whose automaton holds the empty needle (Automaton.hs:373-376, 502-519), by byte comparison alone: after every
    successful goto, i.e. wherever a non-empty PREFIX of some casing of some needle ends inside its haystack, the state's values are folded: the root's (the
    empty needle) and one per needle that ends there.  Returns (haystack, end_pos, n_values) in batch order, end_pos relative to the haystack as in am_match."""
    import alfred_margaret_amd as am
    t = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    offs = np.asarray(offs, dtype=np.int64)
    whole, prefixes = set(), set()
    for nd in needles:
        for c in ((am.needle_casings(nd) if case else [nd.encode("utf-8")]) if nd else []):
            s = c.decode("utf-8")
            whole.add(c)
            prefixes.update(s[:k].encode("utf-8") for k in range(1, len(s) + 1))
    folded, ends = np.zeros(len(t), dtype=bool), np.zeros(len(t), dtype=np.uint8)
    for p in sorted(prefixes):
        if len(p) > len(t):
            continue
        m = t[:len(t) - len(p) + 1] == p[0]
        for k in range(1, len(p)):
            m &= t[k:len(t) - len(p) + 1 + k] == p[k]
        e = np.flatnonzero(m) + len(p) - 1                         # last byte of every occurrence
        e = e[e - len(p) + 1 >= offs[np.searchsorted(offs, e, side="right") - 1]]      # ... that starts in the haystack it ends in
        folded[e] = True
        if p in whole:
            ends[e] += 1
    g = np.flatnonzero(folded)
    hay = np.searchsorted(offs, g, side="right") - 1
    n_values = ends[g].astype(np.int64) + (1 if "" in needles else 0)
    keep = n_values > 0
    return hay[keep], (g - offs[hay] + 1)[keep], n_values[keep]


def dense_placements(case, needles, text, offs, unit_bytes):
    """How often a batch holds what k_dense can get wrong: {placement: count}.  `first` = a multi-byte code point that is (a casing of) a first code point of a needle."""
    t = np.frombuffer(text, dtype=np.uint8) if not isinstance(text, np.ndarray) else text
    offs = np.asarray(offs, dtype=np.int64)
    firsts = [nd[0] for nd in needles if nd]
    hay, end, _ = dense_reference(case, [""] + firsts, t, offs)
    g = offs[hay] + end - 1                                        # last bytes of the first code points
    multi = g[(t[g] & 0xC0) == 0x80]
    hay_ends = offs[1:][np.diff(offs) > 0] - 1
    word_of_start = offs[:-1] // DENSE_WORD
    starts_per_word = np.bincount(word_of_start[offs[:-1] < len(t)].astype(np.int64))
    empty_inside = (np.diff(offs) == 0) & (offs[:-1] % DENSE_WORD != 0) & (offs[:-1] < len(t))
    n_cp = int(((t & 0xC0) != 0x80).sum())
    return {"first ends a word": int((multi % DENSE_WORD == DENSE_WORD - 1).sum()), "first ends on the first byte of a word": int((multi % DENSE_WORD == 0).sum()),
            "first ends a unit": int((multi % unit_bytes == unit_bytes - 1).sum()),
            "first ends a haystack and a word": int(np.intersect1d(multi[multi % DENSE_WORD == DENSE_WORD - 1], hay_ends).size),
            "words with three haystacks": int((starts_per_word >= 3).sum()), "empty haystacks inside a word": int(empty_inside.sum()),
            "first share": len(g) / max(n_cp, 1)}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Needle families that put an automaton's image into each cell of launch_sf_t's rule (csrc/am_kernels.hip: ILP, LW, SHORT, CHILDREN), and texts that hold what a
# k_sf instantiation can get wrong: verbatim needles, near misses that pass the 4-byte suffix filter and die later, cuts inside needles and next to KiB boundaries.
# tests/test_sf_variants_cpu.py checks on the CPU that every family sits in the cell it claims; tests/test_gpu_sf_variants.py feeds them to the kernels.

SF_FAMILIES = {"small": 2000, "mid": 34000, "large": 60000, "dict": 20000, "forked": 40000}      # name -> needles; "<name>+short" adds SF_SHORT_NEEDLES
SF_SHORT_NEEDLES = ["~", "q7", "z9k", "ж", "語", "é5"]                          # 1, 2, 3 bytes of ASCII; 2, 3, 3 bytes with a multi-byte code point; none of their rare bytes is in SF_FILLER
SF_SHORT_UPPER = ["~", "Q7", "Z9K", "Ж", "語", "É5"]
SF_FILLER = "abcdefghijklmnopqrstuvwxyz" + "ABCDEFGHIJKLMNOPQRSTUVWXYZ" + " ,.0123" + "яЯåÅσΣ𝄞ß"
SF_SWAP = {1: "xv", 2: "дю", 3: "本日", 4: "💩𝄢"}                             # a near miss replaces a code point by another of the same byte length
_SF_NEEDLES = {}


def sf_family_needles(family):
    """The needles of a family, lower case, distinct, deterministic.  small / mid / large: random a-z words of 5-12 letters plus 200 lower-cased words of 2-6 code points
    (>= 4 bytes) over the non-ASCII alphabets of ALPHABETS; dict: the first 20 000 needles of the natural-language benchmark dictionary; forked: 20 000 random 4-letter
    stems, each behind two different letters and 0-6 random ones before those -- few suffix keys (a filter below 2^15 words), every suffix node heavy (a suffix table
    beyond 2^15 buckets once the child entries are in it)."""
    if family not in _SF_NEEDLES:
        name, _, short = family.partition("+")
        assert name in SF_FAMILIES and short in ("", "short"), family
        if name == "dict":
            from alfred_margaret_amd import synth
            ns = list(synth.needles_for("natural_100k_10GiB")[:SF_FAMILIES[name]])
        elif name == "forked":
            rng, az, stems, seen = random.Random("sf-forked"), "abcdefghijklmnopqrstuvwxyz", set(), set()
            while len(stems) < SF_FAMILIES[name] // 2:
                stems.add("".join(rng.choice(az) for _ in range(4)))
            for s in sorted(stems):
                for f in rng.sample(az, 2):
                    seen.add("".join(rng.choice(az) for _ in range(rng.randint(0, 6))) + f + s)
            ns = sorted(seen)
            rng.shuffle(ns)
        else:
            rng = random.Random("sf-" + name)
            seen = set()
            while len(seen) < 200:
                w = oracle.lower_utf8("".join(rng.choice(rng.choice(ALPHABETS[1:3])) for _ in range(rng.randint(2, 6)))).decode("utf-8")
                if len(w.encode("utf-8")) >= 4 and not w.isascii():
                    seen.add(w)
            while len(seen) < 200 + SF_FAMILIES[name]:
                seen.add("".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(5, 12))))
            ns = sorted(seen)
            rng.shuffle(ns)
        _SF_NEEDLES[family] = ns + (SF_SHORT_NEEDLES if short else [])
    return _SF_NEEDLES[family]


def _sf_upper_partners():
    """{lower-case code point: [code points that lower to it]} over the letters of ALPHABETS (U+212A -> k, U+212B -> å, ẞ -> ß change the byte length) and A-Z."""
    out = {}
    for c in sorted(set("".join(ALPHABETS)) | set("ABCDEFGHIJKLMNOPQRSTUVWXYZ")):
        low = oracle.lower_utf8(c).decode("utf-8")
        if low != c and len(low) == 1:
            out.setdefault(low, []).append(c)
    return out


def _cp_floor(t, c):
    while 0 < c < len(t) and (t[c] & 0xC0) == 0x80:
        c -= 1
    return c


def sf_near_miss(rng, needle, in_suffix):
    """`needle` with one code point replaced by another of the same byte length (one byte, for the a-z words): inside its last four bytes, where the filter or the
    probe refuses it, or before them, where it passes both and dies in the resolve.  A needle too short for the latter is changed in its suffix."""
    cps = list(needle)
    ends = np.cumsum([len(c.encode("utf-8")) for c in cps])
    total = int(ends[-1])
    inside = [i for i in range(len(cps)) if ends[i] > total - 4]
    before = [i for i in range(len(cps)) if ends[i] <= total - 4]
    i = rng.choice(inside if in_suffix or not before else before)
    a, b = SF_SWAP[len(cps[i].encode("utf-8"))]
    cps[i] = b if cps[i] == a else a
    return "".join(cps)


def sf_text(family, case, n_bytes, seed=0):
    """(text, offsets np.int64) of exactly n_bytes of valid UTF-8 for a family: about 30 % verbatim needles (under IgnoreCase a third of them with random upper-casing
    through every partner of _sf_upper_partners), 20 % near misses (half of them changed before the last four bytes), the rest filler over SF_FILLER; every 40th piece is
    one of SF_SHORT_NEEDLES (or its upper case), whether or not the family holds them.  The haystacks: ragged_cuts' pattern, cuts at multiples of 1 024 +- 1, cuts in
    the middle of forty planted needles, empty haystacks, and at the end three haystacks of filler only and three of near misses only."""
    rng = random.Random("sf-text-%s-%d-%d-%d" % (family, case, n_bytes, seed))
    needles = sf_family_needles(family.partition("+")[0])
    partners = _sf_upper_partners()

    def filler():
        return "".join(rng.choice(SF_FILLER) for _ in range(rng.randint(1, 24)))

    def cased(nd):
        if not case or rng.random() < 0.67:
            return nd
        return "".join(rng.choice(partners[c]) if c in partners and rng.random() < 0.4 else c for c in nd)

    tail = [filler().encode("utf-8") + filler().encode("utf-8") for _ in range(3)]
    tail += ["".join(sf_near_miss(rng, rng.choice(needles), k % 2 == 0) for k in range(4)).encode("utf-8") for _ in range(3)]
    room = n_bytes - sum(len(t) for t in tail)
    assert room > 2048, n_bytes
    parts, planted, at, k = [], [], 0, 0
    while True:
        k += 1
        r = rng.random()
        if k % 40 == 0:
            i = rng.randrange(len(SF_SHORT_NEEDLES))
            p = (SF_SHORT_UPPER[i] if case and rng.random() < 0.5 else SF_SHORT_NEEDLES[i]).encode("utf-8")
        elif r < 0.40:
            p = cased(rng.choice(needles)).encode("utf-8")
            planted.append((at, len(p)))
        elif r < 0.67:
            p = sf_near_miss(rng, rng.choice(needles), rng.random() < 0.5).encode("utf-8")
        else:
            p = filler().encode("utf-8")
        if at + len(p) > room:
            break
        parts.append(p)
        at += len(p)
    parts.append(b"X" * (room - at))
    body = b"".join(parts)
    t = np.frombuffer(body, dtype=np.uint8)
    cuts = [ragged_cuts(t, rng, big=1 << 20)]
    kib = [k * 1024 + d for k in rng.sample(range(1, room // 1024), min(12, room // 1024 - 1)) for d in (-1, 1)]
    inside = [s + n // 2 for s, n in rng.sample(planted, min(40, len(planted)))]
    cuts.append(np.asarray([_cp_floor(t, c) for c in kib + inside], dtype=np.int64))
    offs = np.sort(np.concatenate(cuts))
    offs = np.concatenate([offs, room + np.cumsum([len(x) for x in tail])]).astype(np.int64)
    text = body + b"".join(tail)
    assert len(text) == n_bytes and offs[0] == 0 and offs[-1] == n_bytes
    return text, offs


def sf_oracle_records(machine, case, text, offs):
    """The oracle over every haystack of a batch: (haystack, matchPos, value) as arrays, in fold order."""
    hay, pos, val = [], [], []
    for i in range(len(offs) - 1):
        if offs[i + 1] > offs[i]:
            p, v = machine.run_list(case, text, int(offs[i]), int(offs[i + 1] - offs[i]))
            if len(p):
                hay.append(np.full(len(p), i, np.uint32)); pos.append(p); val.append(v)
    if not hay:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    return np.concatenate(hay), np.concatenate(pos), np.concatenate(val)


def sf_expand(hay, state, end, values_off, values):
    """Records -> (haystack, matchPos, value) arrays in fold order (expand_records, vectorised)."""
    st = np.asarray(state, dtype=np.int64)
    lens = (values_off[st + 1] - values_off[st]).astype(np.int64)
    n = int(lens.sum())
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    within = np.arange(n) - np.repeat(np.cumsum(lens) - lens, lens)
    return np.repeat(np.asarray(hay, np.uint32), lens), np.repeat(np.asarray(end, np.uint64), lens), values[np.repeat(values_off[st].astype(np.int64), lens) + within]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# LONG needles: 17 bytes to 66 000, on every scan and Replacer route.  What depends on the longest needle:
#   k_sf resolve (csrc/am_image.h): the slot line settles a needle of up to 4 + 1 + 16 = 21 bytes (sf_resolve_head :727-734: the 4-byte suffix, the single
#     edge's selector byte and a label of at most kMaxSkip = 16); every step of sf_resolve_walk consumes at most 1 + 16 = 17 bytes (:847, :856), which it reads
#     back from global memory at gpos - depth (:809, :835), guarded at the haystack's start by depth + 1 + skip > avail (:847), avail a u32 clamp (:676).
#   the walker queue (csrc/am_kernels.hip): count and emit park a walker that is not done after kSfWqIters = 2 steps (:70, :256-258); walk_parked (:173) takes
#     it to the end; a parked walker that finds nothing leaves state == kNone in its slot (:302), one that finds a deeper end patches its record (:198).
#   k_dfa / k_ac warm-up, range_window's overlap, the segments of am_run and the Replacer's reach ov (csrc/am_replacer.cpp:387, :658, :835-838).
# So, for a needle that is the ONLY path from its 4-byte suffix (the independent random needles below): 21 | 22 bytes = the slot line settles it | the first
# walk step, 38 | 39 = one step | two, 55 | 56 = two steps (inline) | a third (parked).  The suffixes of one base string at the same lengths are a CHAIN of
# needle ends instead: every end splits the edge, so the walk to the 57-byte needle passes nine shallower ends, parks after the second and replaces `prior`.
# tests/test_long_needles_cpu.py checks on the CPU that all of this is what it claims; tests/test_gpu_long_needles.py feeds it to the kernels.

LONG_ALPHABETS = ("ab", "abcdefgh", "abkåßi", "ak𝄞яß")          # 1- to 4-byte code points; k å ß i have the partners U+212A, U+212B, ẞ, İ whose lower-casing changes the byte length
LONG_SHORT_LENGTHS = (17, 20, 21, 22, 37, 38, 39, 55, 56, 57)
LONG_POW_LENGTHS = tuple(p + d for p in (256, 1024, 2048, 4096, 8192) for d in (-1, 0, 1))
LONG_STEP_LENGTHS = LONG_SHORT_LENGTHS + LONG_POW_LENGTHS
LONG_SLOT_LINE = 4 + 1 + 16            # am_image.h:727-734
LONG_STEP = 1 + 16                     # am_image.h:856, kMaxSkip
LONG_PARK_AFTER = 2                    # am_kernels.hip:70 kSfWqIters
LONG_BEYOND = (16500, 66000)           # more than the light configuration's 16 chunks (am_kernels.hip:64); more than 65 535 and than a 64-chunk unit (:69)
LONG_FORK_DEPTH = 700                  # code points of the deep forks' shared suffix
LONG_FANOUTS = (2, 4, 5, 7)            # <= 4 edges are inline in the node record, more take a displaced row (am_image.h:812-818)
LONG_BATCH_LIMIT = 1 << 20
LONG_MISS_DISTANCES = (1, 5, 21, 22, 38, 39, 56)
LONG_KIB_ENDS = (-1, 0, 1, 4, 5)
LONG_FILLER = "mnopqrstuvwxyz ,."     # one byte each, in no alphabet and nobody's case partner
_LONG_SETS = {}
_LONG_TEXTS = {}


def _exact_bytes(rng, alphabet, n_bytes):
    """Random code points of `alphabet` that add up to exactly n_bytes (every alphabet holds a one-byte code point)."""
    out, left = [], n_bytes
    while left:
        c = rng.choice([c for c in alphabet if len(c.encode("utf-8")) <= left])
        out.append(c)
        left -= len(c.encode("utf-8"))
    return "".join(out)


def _chain_base(rng, alphabet, lengths):
    """One string of max(lengths) bytes whose suffix of exactly L bytes starts on a code point, for every L of lengths."""
    out, have = "", 0
    for ln in sorted(lengths):
        out = _exact_bytes(rng, alphabet, ln - have) + out
        have = ln
    return out


def _suffix_bytes(s, n_bytes):
    b = s.encode("utf-8")
    assert n_bytes <= len(b) and (n_bytes == len(b) or (b[len(b) - n_bytes] & 0xC0) != 0x80), n_bytes
    return b[len(b) - n_bytes:].decode("utf-8")


def _fork_code_points(alphabet, k):
    """k code points with k different LAST bytes (the walk goes backwards: the last byte is the edge's selector): the alphabet's, then a-h."""
    out = []
    for c in alphabet + "cdefgh":
        if c.encode("utf-8")[-1] not in [d.encode("utf-8")[-1] for d in out]:
            out.append(c)
    assert len(out) >= k, (alphabet, k)
    return out[:k]


def long_needle_sets():
    """{name: needles}, lower case (the same list serves CaseSensitive and IgnoreCase), deterministic.  No needle is ever dropped: duplicates are kept, and
    tests/test_long_needles_cpu.py holds every list to the byte lengths it is built for.
      steps/<alphabet>    suffixes of one base string at LONG_STEP_LENGTHS bytes, independent random needles of the same lengths, the 57- and the 1024-byte suffix twice
      beyond/<alphabet>   16 500 and 66 000 bytes, their suffixes of 1 025 and 8 193 bytes, their 70-byte prefixes
      forks/<alphabet>    2, 4, 5, 7 different code points in front of a shared suffix of 700 code points and of a 9-byte suffix, and continuations of 1-40 code points
      periodic            "ab" * 4000, "ab" * 12, "ba" * 30"""
    if _LONG_SETS:
        return _LONG_SETS
    for alphabet in LONG_ALPHABETS:
        rng = random.Random("long-steps-" + alphabet)
        base = _chain_base(rng, alphabet, LONG_STEP_LENGTHS)
        chain = [_suffix_bytes(base, ln) for ln in LONG_STEP_LENGTHS]
        alone = []
        for ln in LONG_STEP_LENGTHS:
            while True:
                s = _exact_bytes(rng, alphabet, ln)
                if s[-4:] != base[-4:] and all(s[-4:] != a[-4:] for a in alone):       # last four code points of its own: the only path from its suffix
                    break
                if len(alphabet) == 2 and s != _suffix_bytes(base, ln):               # ("ab" has 16 such endings for 25 needles: there they share them)
                    break
            alone.append(s)
        _LONG_SETS["steps/" + alphabet] = chain + alone + [_suffix_bytes(base, 57), _suffix_bytes(base, 1024)]
    for alphabet in (LONG_ALPHABETS[0], LONG_ALPHABETS[3]):
        rng = random.Random("long-beyond-" + alphabet)
        ns = []
        for total in LONG_BEYOND:
            base = _chain_base(rng, alphabet, (1025, 8193, total))
            head = base.encode("utf-8")[:70]
            while (base.encode("utf-8")[len(head)] & 0xC0) == 0x80:
                head = head[:-1]
            head = head.decode("utf-8")
            ns += [base, _suffix_bytes(base, 1025), _suffix_bytes(base, 8193), head + "a" * (70 - len(head.encode("utf-8")))]
        _LONG_SETS["beyond/" + alphabet] = ns
    for alphabet in LONG_ALPHABETS[1:]:
        rng = random.Random("long-forks-" + alphabet)
        ns = []
        for shared in ("".join(rng.choice(alphabet) for _ in range(LONG_FORK_DEPTH)), _exact_bytes(rng, alphabet[:2], 9)):
            for k in LONG_FANOUTS:
                sep = "".join(rng.choice(alphabet) for _ in range(3))                    # the forks of different fan-outs do not share their suffix
                stem = sep + shared
                forks = [c + stem for c in _fork_code_points(alphabet, k)]
                ns += forks
                ns += ["".join(rng.choice(alphabet) for _ in range(n)) + forks[i % k] for i, n in enumerate((1, 17, 40))]
        _LONG_SETS["forks/" + alphabet] = ns
    _LONG_SETS["periodic"] = ["ab" * 4000, "ab" * 12, "ba" * 30]
    return _LONG_SETS


def _long_treatment(n_bytes, alone):
    """What the text holds for a needle of n_bytes: (near-miss distances from the end + "middle" / "first", ends relative to a multiple of 1 024, start placement,
    cuts).  Everything up to 1 025 bytes; above, fewer near misses and placements, so that a batch stays within LONG_BATCH_LIMIT (the kinds all stay)."""
    if n_bytes <= 1025:
        return LONG_MISS_DISTANCES + ("middle", "first"), (0, 5) if alone else LONG_KIB_ENDS, True, ("first", "half")
    if alone:
        return (56,), (0,), False, ("half",)
    if n_bytes <= 2049:
        return (1, 56, "middle", "first"), (-1, 0), True, ("first", "half")
    if n_bytes <= 16500:
        return (56, "first"), (0,), True, ("half",)
    return (56, "first"), (0,), False, ("half",)


def long_near_miss(needle, where):
    """`needle` with the code point that holds the byte `where` bytes before its end ("middle": its middle byte, "first": its first code point) swapped for
    another of the same byte length (SF_SWAP); None where the needle is shorter than that."""
    cps = list(needle)
    ends = np.cumsum([len(c.encode("utf-8")) for c in cps])
    total = int(ends[-1])
    if where == "first":
        i = 0
    elif where == "middle":
        i = int(np.searchsorted(ends, total // 2, side="right"))
    elif where > total:
        return None
    else:
        i = int(np.searchsorted(ends, total - where, side="right"))
    a, b = SF_SWAP[len(cps[i].encode("utf-8"))]
    cps[i] = b if cps[i] == a else a
    return "".join(cps)


class LongText:
    """text (bytes), offs (np.int64), and what was planted: items = [(kind, needle index, haystack index, detail)] with kind in "whole", "cased", "minus first",
    "plus one", "cut", "near miss", "ends at", "starts at", "periodic", "mixed", "empty"."""

    def __init__(self, text, offs, items):
        self.text, self.offs, self.items = text, offs, items

    def hays(self):
        return [self.text[self.offs[i]:self.offs[i + 1]] for i in range(len(self.offs) - 1)]


def long_text_parts(name):
    """Batches the text of a set comes in: the steps sets take two, needles of up to 2 049 bytes and the longer ones, to stay within LONG_BATCH_LIMIT."""
    return 2 if name.startswith("steps/") else 1


def long_needle_plan(name, case, seed=0, part=0):
    """The LongText behind long_needle_text."""
    key = (name, case, seed, part)
    assert 0 <= part < long_text_parts(name)
    if key in _LONG_TEXTS:
        return _LONG_TEXTS[key]
    needles = long_needle_sets()[name]
    rng = random.Random("long-text-%s-%d-%d-%d" % key)
    partners = _sf_upper_partners()
    chain_len = len(LONG_STEP_LENGTHS) if name.startswith("steps/") else 0
    hays, items = [], []
    at = [0]

    def add(kind, i, detail, *pieces):
        for p in pieces:
            b = p.encode("utf-8") if isinstance(p, str) else p
            items.append((kind, i, len(hays), detail))
            hays.append(b)
            at[0] += len(b)

    def fill(n):
        return "".join(rng.choice(LONG_FILLER) for _ in range(n))

    def cased(nd):
        share = rng.uniform(0.3, 0.4)
        return "".join(rng.choice(partners[c]) if c in partners and rng.random() < share else c for c in nd)

    for i, nd in enumerate(needles):
        nb = len(nd.encode("utf-8"))
        if long_text_parts(name) == 2 and (nb > 2049) != (part == 1):
            continue
        alone = name.startswith("steps/") and chain_len <= i < 2 * chain_len
        misses, kib_ends, start_at, cuts = _long_treatment(nb, alone)
        add("whole", i, None, nd)
        if case:
            add("cased", i, None, cased(nd))
        add("minus first", i, None, nd[1:])
        add("plus one", i, None, rng.choice(LONG_FILLER + nd[0]) + nd)
        for cut in cuts:                                            # (on a code point: a haystack is valid UTF-8) after the first code point, after the first half
            k = 1 if cut == "first" else len(nd) // 2
            add("cut", i, cut, nd[:k], nd[k:])
        for where in misses:
            nm = long_near_miss(nd, where)
            if nm is not None:
                add("near miss", i, where, nm)
        for d in kib_ends:                                          # the byte behind the needle's last is byte k * 1024 + d of the batch
            pad = (d - at[0] - nb) % 1024
            pad += 1024 if pad < 8 else 0
            add("ends at", i, d, fill(pad) + nd)
            assert (at[0] - d) % 1024 == 0
        if start_at:                                                # the needle's first byte is byte k * 1024 - 1 of the batch
            pad = (-1 - at[0]) % 1024
            pad += 1024 if pad < 8 else 0
            add("starts at", i, -1, fill(pad) + nd + fill(5))
    if name == "periodic":
        add("periodic", 0, None, "ab" * (32 << 10))
    for _ in range(3):
        add("empty", -1, None, "")
    room = min(256 << 10, LONG_BATCH_LIMIT - at[0])
    assert room >= (96 << 10), (name, case, at[0])
    small = [i for i, nd in enumerate(needles) if len(nd.encode("utf-8")) <= 8193]
    parts, size = [], 0
    while True:
        r, i = rng.random(), rng.choice(small)
        nd = needles[i]
        if r < 0.45:
            p = cased(nd) if case and rng.random() < 0.5 else nd
        elif r < 0.75:
            p = long_near_miss(nd, rng.choice(LONG_MISS_DISTANCES + ("middle", "first"))) or nd[1:]
        else:
            p = fill(rng.randint(1, 40))
        p = p.encode("utf-8")
        if size + len(p) > room:
            break
        parts.append(p)
        size += len(p)
    add("mixed", -1, None, b"".join(parts))
    text = b"".join(hays)
    offs = np.concatenate([[0], np.cumsum([len(h) for h in hays])]).astype(np.int64)
    assert len(text) <= LONG_BATCH_LIMIT, (name, case, len(text))
    _LONG_TEXTS[key] = LongText(text, offs, items)
    return _LONG_TEXTS[key]


def long_needle_text(name, case, seed=0, part=0):
    """(text, offsets np.int64) for the set `name` (batch `part` of long_text_parts(name)), at most LONG_BATCH_LIMIT bytes, one haystack per planted piece.  For every needle: the needle alone; under
    IgnoreCase also with 30-40 % of its code points replaced by an upper-case partner (K for k: up to three times the bytes); without its first code point; with
    one code point in front; cut in two haystacks after its first code point and after its first half; near misses (long_near_miss) 1, 5, 21, 22, 38, 39, 56 bytes
    from the end, in the middle and at the first code point; ending at byte k * 1024 + d of the batch for d in LONG_KIB_ENDS, and starting at k * 1024 - 1
    (_long_treatment thins these out above 1 025 bytes).  Then 64 KiB of "ab" (periodic only), three empty haystacks and one mixed haystack of needles, near
    misses and filler that takes the room left, 256 KiB at most."""
    t = long_needle_plan(name, case, seed, part)
    return t.text, t.offs


def long_needle_unit_text(total, unit_bytes, seed=0):
    """(needles, text, offs) for batches whose work units hold several chunks: the 1 025-, 8 193- and 16 500-byte needles of beyond/ab placed so that they end
    1, 5, half their length and all but one byte behind a unit boundary, alone and behind a near miss; filler in between; haystacks of 0 to 3 units."""
    rng = random.Random("long-units-%d-%d-%d" % (total, unit_bytes, seed))
    ns = long_needle_sets()["beyond/ab"]
    picked = [n for n in ns if len(n) in (1025, 8193, 16500)]
    assert sorted(set(len(n) for n in picked)) == [1025, 8193, 16500]
    buf = np.frombuffer(("".join(rng.choice(LONG_FILLER) for _ in range(4096)) * (total // 4096 + 1))[:total].encode(), dtype=np.uint8).copy()
    n_units = total // unit_bytes
    per = 34000 // unit_bytes + 2                                  # units between two placements: they never overlap
    u, k, placed = per, 0, 0
    while u < n_units - 1:
        nd = picked[k % len(picked)]
        behind = (1, 5, len(nd) // 2, len(nd) - 1)[(k // len(picked)) % 4]
        end = u * unit_bytes + behind
        piece = nd if k % 5 else long_near_miss(nd, 56) + nd
        assert end - len(piece) >= (u - per + 1) * unit_bytes and end <= total
        buf[end - len(piece):end] = np.frombuffer(piece.encode(), dtype=np.uint8)
        placed += 1
        u += per
        k += 1
    assert placed >= 24, (total, unit_bytes, placed)               # every needle at every distance, twice
    cuts, c = [0], 0
    while c < total:
        c = min(total, c + rng.choice((0, 1, unit_bytes // 2 + 3, unit_bytes, 3 * unit_bytes + 1, 40 * unit_bytes)))
        cuts.append(c)
    return ns, buf.tobytes(), np.asarray(cuts, dtype=np.int64)


# ---- Replacer: a match that a replacement COMPLETES, |L| bytes to its left and |R| to its right ------------------------------------------------------------
# The one-kernel route takes a replacer while round_up_64(2 ov + longest replacement + 16) <= 4096 (am_replacer.cpp:837-838), ov = the longest needle in bytes
# for CaseSensitive replacers and 4 * code points + 4 under IgnoreCase (:835-836).  The replacements here are one byte long: 2 ov + 17 <= 4096, ov <= 2039.
LONG_RP_OV_LIMIT = (4096 - 16 - 1) // 2                       # 2039: the largest reach the one-kernel route takes with one-byte replacements
LONG_RP_CS_LIMIT = (LONG_RP_OV_LIMIT, LONG_RP_OV_LIMIT + 1)   # needle BYTES at and above the limit (CaseSensitive): 2039, 2040
LONG_RP_IC_LIMIT = ((LONG_RP_OV_LIMIT - 4) // 4, (LONG_RP_OV_LIMIT - 4) // 4 + 1)      # needle CODE POINTS at and above it (IgnoreCase): 508 (ov 2036), 509 (ov 2040)


def long_route_cap(case, pairs):
    """round_up_64(2 ov + longest replacement + 16) of am_replacer.cpp:837."""
    return (2 * reach(case, pairs) + max(len(r.encode("utf-8")) for _, r in pairs) + 16 + 63) // 64 * 64


class LongReplacerCase:
    """pairs over docs (str); `expect` the final texts, `passes` the scans the longest-running document needs (Replacer.hs:219-242), `fits[i]`: document i's first
    re-scan window (am_rplds.hip:262-266) is within LDS_WIN."""

    def __init__(self, name, case, pairs, docs, expect, passes):
        self.name, self.case, self.pairs, self.docs, self.expect, self.passes = name, case, pairs, docs, expect, passes
        self.ov, self.cap = reach(case, pairs), long_route_cap(case, pairs)
        self.fits = []
        for d in docs:
            b = d.encode("utf-8")
            ms = b.index(b"@")
            self.fits.append(min(ms + 1 + self.ov, len(b)) - max(ms - self.ov, 0) <= LDS_WIN)

    def __repr__(self):
        return "LongReplacerCase(%s)" % self.name


def _long_rp_case(name, case, nl, nr, rng, alphabet="abcdefgh", upper=False):
    """N = L + "#" + R with |L| = nl and |R| = nr code points: [("@", "#"), (N, "!"), NEVER] over L + "@" + R, bare, inside filler, and at the text's start / end."""
    left = "".join(rng.choice(alphabet) for _ in range(nl))
    right = "".join(rng.choice(alphabet) for _ in range(nr))
    pairs = [("@", "#"), (left + "#" + right, "!"), NEVER]
    if upper:
        partners = _sf_upper_partners()
        shown = "".join(rng.choice(partners[c]) if c in partners and rng.random() < 0.5 else c for c in left)
        assert shown != left
    else:
        shown = left
    pad = "x" * (nl + nr + 40)
    docs = [shown + "@" + right, pad + shown + "@" + right + pad, shown + "@" + right + pad, pad + shown + "@" + right, "x" * 7 + shown + "@" + right + "x" * 9]
    expect = [b"!", (pad + "!" + pad).encode(), ("!" + pad).encode(), (pad + "!").encode(), b"x" * 7 + b"!" + b"x" * 9]
    return LongReplacerCase(name, case, pairs, docs, expect, 3)


def long_needle_replacer_cases():
    """|L| = |R| in 8, 100, 223, 224, 500, 1000, 3000 code points, both case modes; the two needle lengths on either side of the host's route limit in each mode
    (LONG_RP_CS_LIMIT in bytes, LONG_RP_IC_LIMIT in code points); all the length in L, all of it in R; IgnoreCase with L written in K / İ / ẞ / Å; and a chain of
    three pairs in which every replacement completes the next needle."""
    out = []
    for case in (0, 1):
        tag = "IC" if case else "CS"
        rng = random.Random("long-rp-%d" % case)
        for n in (8, 100, 223, 224, 500, 1000, 3000):
            out.append(_long_rp_case("%d+%d %s" % (n, n, tag), case, n, n, rng))
        for total in (LONG_RP_IC_LIMIT if case else LONG_RP_CS_LIMIT):
            nl = (total - 1) // 2
            out.append(_long_rp_case("limit %d %s" % (total, tag), case, nl, total - 1 - nl, rng))
        out.append(_long_rp_case("all left %s" % tag, case, 400, 0, rng))
        out.append(_long_rp_case("all right %s" % tag, case, 0, 400, rng))
        # a chain: "@" -> "#" completes N1 -> "$" completes N2 -> "%" completes N3 -> "!"
        parts = ["".join(rng.choice("abcdefgh") for _ in range(n)) for n in (60, 60, 150, 150, 300, 300)]
        l1, r1, l2, r2, l3, r3 = parts
        pairs = [("@", "#"), (l1 + "#" + r1, "$"), (l2 + "$" + r2, "%"), (l3 + "%" + r3, "!"), NEVER]
        core = l3 + l2 + l1 + "@" + r1 + r2 + r3
        pad = "x" * 700
        out.append(LongReplacerCase("chain %s" % tag, case, pairs, [core, pad + core + pad, core + pad], [b"!", (pad + "!" + pad).encode(), ("!" + pad).encode()], 5))
    rng = random.Random("long-rp-upper")
    out.append(_long_rp_case("upper 100+100 IC", 1, 100, 100, rng, alphabet="kiåßab", upper=True))
    out.append(_long_rp_case("upper 400+8 IC", 1, 400, 8, rng, alphabet="kiåß", upper=True))
    return out


def replacer_passes(case, pairs, text):
    """(final text, scans) of Replacer.run restated with the oracle's automaton (Replacer.hs:219-242): a scan per pass; the pass replaces the matches of the best
    priority below the threshold; the loop ends with a scan that finds none, or with the lowest priority."""
    m = oracle.Machine([oracle.lower_utf8(n) if case else n.encode("utf-8") for n, _ in pairs])
    text = text.encode("utf-8") if isinstance(text, str) else text
    threshold, scans = 1, 0
    while True:
        scans += 1
        _, val = m.run_list(case, text)
        below = [-int(v) for v in val if -int(v) < threshold]
        if not below:
            return text, scans
        p = max(below)
        text = oracle.Replacer(case, [pairs[-p]]).run(text)
        if p == 1 - len(pairs):
            return text, scans
        threshold = p


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The table walk's storage tiers (csrc/am_dfa.hip dfa_step): a mid-size automaton whose DFA section leaves LDS in every direction -- rows beyond the LDS rows, columns
# beyond the LDS and the hot columns, records of both kinds beyond their LDS share, more than 16 384 states (k_dfa_place's 4-byte entries carry a tag), states with
# 14, 15, 16 and more values (kDfaEndLookUp) -- and a plain walk of the section that says which tier answered every step.  tests/test_dfa_tiers_cpu.py holds the walk
# to the oracle and the counts to floors; tests/test_gpu_dfa_tiers.py feeds the same automaton and text to k_dfa under every launch shape.

DFA_TIER_ALPHABET = "abcdefghijklmnopqrstuvwxyz" + "ABCDEFGHIJKLMNOPQRSTUVWXYZ" + "0123456789" + " ,.-" + "яжщåßσ語💩"
DFA_TIER_FILLER = "_\n"                # in no needle: class 0, the root from everywhere without a load
DFA_TIER_RUN = "Qz" * 9                # its suffixes are needles: k code points into a run, k - 1 of them end (and "zQz" three times more)
DFA_LDS_TWO_PER_CU = (512, 640, 640)   # (rows, single-entry records, two-entry records) a workgroup keeps in LDS, two workgroups per CU (am_dfa.hip:535-538 dfa_launch_shape)
DFA_LDS_ONE_PER_CU = (1008, 2048, 1024)    # one workgroup per CU with all of its LDS (am_dfa.hip:535-538)
DFA_LDS_COLS = 32                      # kLdsLog2Cols (am_dfa.hip:57): LDS holds columns 1 .. 32 of its rows
DFA_END_LOOK_UP = 15                   # kDfaEndLookUp (am_image.h:197): end bits of a list of 15 values and more; the count then reads out[]
DFA_PLACE_SLOTS = 8192                 # k_dfa_place's 4-byte entries (am_dfa.hip:465: slot = st & 8191, the rest is the tag)
DFA_PLACE_MUL, DFA_PLACE_SHIFT = 0x9E3779B1, 20      # ... and its 8-byte entries (am_dfa.hip:469: 4 096 slots under a hash)
DFA_SUPER_ROOM = 4096 - 1024           # kDfaSuper - kDfaSuperReserve (am_dfa.hip:52-53): tokens a superblock takes before its wavefront draws the next one
DFA_TIERS = ("lds_rows", "lds_row_col_above_32", "hot", "cold", "single_lds", "single_global", "single_ahead", "two_lds", "two_global", "two_first", "two_second", "two_leans")


def dfa_tier_needles(seed=0):
    """6 000 random needles of 2-9 code points over DFA_TIER_ALPHABET (one to four bytes a code point, both cases of a-z), the 17 suffixes of DFA_TIER_RUN from 18 code
    points down to 2, and "zQz" three times more: k code points into a run of QzQz..., k - 1 suffixes end (k <= 18) and from k = 3 on the three "zQz" too, so that a run
    entered at Q reports 1, 6, 8, ... 14, 16, 18, 20 values and a run entered at z (a haystack cut after an odd number of its code points) 5, 7, ... 15, 17, 19:
    14, 15 and 16 lie on both sides of kDfaEndLookUp.  CaseSensitive as they are; an IgnoreCase test lower-cases them as the other tests do."""
    rng = random.Random("dfa-tiers-%d" % seed)
    out = ["".join(rng.choice(DFA_TIER_ALPHABET) for _ in range(rng.randint(2, 9))) for _ in range(6000)]
    return out + [DFA_TIER_RUN[i:] for i in range(17)] + ["zQz"] * 3


def _dfa_upper(rng, s):
    return "".join(c.upper() if (rng.random() < 0.25 and len(c.upper()) == 1) else c for c in s)


def dfa_tier_text(needles, case, seed=0, n_bytes=256 << 10, runs_only=False):
    """Ragged haystacks (bytes) of n_bytes in all.  A tile: every needle once -- whole (6 in 10), its last code point changed (2), cut in half (2) --, up to 6 code
    points of filler (the alphabet and DFA_TIER_FILLER) after every other one, 16 runs of DFA_TIER_RUN of which 8 carry a haystack cut after their first 1, 2, 3 or 4 code points; all of it shuffled; under
    IgnoreCase a code point in four upper-cased.  Tiles with fresh shuffles follow each other up to n_bytes.  The text is cut on code-point boundaries into haystacks
    of (0, 0, 1, 5, 40, 300, 3 000, 20 000) bytes at most, and at every cut a run carries.  runs_only: a run (half of them cut) between any two other pieces, and
    an eighth of the needles: a batch that consists mostly of runs split over haystack seams."""
    rng = random.Random("dfa-tier-text-%d-%d-%d-%d" % (case, seed, n_bytes, runs_only))
    alphabet = DFA_TIER_ALPHABET.lower() if case else DFA_TIER_ALPHABET
    blob, forced = bytearray(), []
    while len(blob) < n_bytes:
        tile = []
        for n in (needles[::8] if runs_only else needles):
            r = rng.random()
            s = n if r < 0.6 else n[:-1] + rng.choice(alphabet) if r < 0.8 else n[:len(n) // 2]
            if rng.random() < 0.5:
                s += "".join(rng.choice(alphabet + DFA_TIER_FILLER) for _ in range(rng.randint(0, 6)))
            tile.append((s, None))
        n_runs = len(tile) if runs_only else 16
        tile += [(DFA_TIER_RUN, (1 + i // 2 % 4) if i % 2 else None) for i in range(n_runs)]
        rng.shuffle(tile)
        for s, cut in tile:
            if case:
                s = _dfa_upper(rng, s)
            if cut is not None:
                forced.append(len(blob) + len(s[:cut].encode("utf-8")))
            blob += s.encode("utf-8")
    end = n_bytes
    while end > 0 and (blob[end] & 0xC0) == 0x80:
        end -= 1
    blob = bytes(blob[:end])
    forced = [f for f in forced if f < end]
    hays, p, k = [], 0, 0
    while p < end:
        size = rng.choice((0, 0, 1, 5, 40, 300, 3000, 20000))
        q = min(p + size, end)
        while q < end and q > p and (blob[q] & 0xC0) == 0x80:
            q -= 1
        if size and q == p:                                   # the code point at p is longer than the size drawn: all of it
            q = p + 1
            while q < end and (blob[q] & 0xC0) == 0x80:
                q += 1
        while k < len(forced) and forced[k] <= p:
            k += 1
        if k < len(forced) and forced[k] < q:
            q = forced[k]
        hays.append(blob[p:q])
        p = q
    return hays + [b"", b""]


def dfa_tables(img):
    """The DFA section of an image as arrays (layouts: am_image.h:84-94): next u32[n_rows << log2_classes], hot u32[n_rows << hot_log2], cls u8[256],
    chain u32[n_single + 1][2], chain2 u32[n_states - n_rows - n_single][4], out u32[n_states][2]; "header" = ImgCheck.dfa_header."""
    img = np.frombuffer(bytes(img), dtype=np.uint8)
    h = ImgCheck.dfa_header(img)
    n_two = h["n_states"] - h["n_rows"] - h["n_single"]
    assert h["n_states"] >= 1 and n_two >= 0, h

    def arr(off, count, dtype=np.uint32):
        assert off % 4 == 0 and off + count * np.dtype(dtype).itemsize <= len(img), (off, count, len(img))
        return np.frombuffer(img, dtype=dtype, count=count, offset=off)
    return {"header": h, "next": arr(h["off_next"], h["n_rows"] << h["log2_classes"]), "hot": arr(h["off_hot"], h["n_rows"] << h["hot_log2"]),
            "cls": arr(h["off_cls"], 256, np.uint8), "chain": arr(h["off_chain"], 2 * (h["n_single"] + 1)).reshape(-1, 2),
            "chain2": arr(h["off_chain2"], 4 * n_two).reshape(-1, 4), "out": arr(h["off_out"], 2 * h["n_states"]).reshape(-1, 2)}


def _alias_pairs(keys):
    """pairs of distinct states that share a key"""
    _, n = np.unique(np.asarray(keys, dtype=np.int64), return_counts=True)
    return int((n * (n - 1) // 2).sum())


def dfa_tier_census(img, batch, hot_rows, lds_n1, lds_n2, chunk):
    """A plain walk of the DFA section over `batch` (a list of haystacks), haystack by haystack from the root, that follows dfa_common_step (am_image.h:1109-1126) for
    the answer and dfa_step (am_dfa.hip:123-153) for the place the answer comes from, given what a workgroup keeps in LDS.  Returns
      "tiers"        steps per tier (DFA_TIERS), and "class0", "single_answers", "single_leans" beside them
      "ends"         [(haystack, end_pos)] of every step that ends something, in walk order;  "end_values": the length of each one's list
      "seam_ends"    the ends of 14, 15 or 16 values that lie in another haystack than the one their unit (of `chunk` bytes) starts in
      "groups"       per group of 64 units: {"records", "alias_low" (pairs of distinct end states equal modulo 8 192), "alias_hash" (equal under k_dfa_place's hash)}
    Look-ahead: a single-entry record beyond lds_n1 is answered without a load exactly when the last record load from global memory was of the state before it,
    single-entry as well, and nothing has used what it brought along since.  An image with rare bytes (a class of 0xFF) is refused: this walk has no dfa_rare_step."""
    t = dfa_tables(img)
    h = t["header"]
    cls = t["cls"].tolist()
    if 0xFF in cls:
        raise ValueError("the image has bytes without a column (kDfaRare): dfa_tier_census does not walk them")
    nxt, hot, out_y = t["next"].tolist(), t["hot"].tolist(), t["out"][:, 1].tolist()
    chain, chain2 = t["chain"].tolist(), t["chain2"].tolist()
    n_rows, n_single, l2c, hot_l2 = h["n_rows"], h["n_single"], h["log2_classes"], h["hot_log2"]
    hot_cols = 1 << hot_l2
    c = dict.fromkeys(DFA_TIERS + ("class0", "single_answers", "single_leans"), 0)
    ends, end_values, end_states, end_global, seam_ends = [], [], [], [], []
    starts = np.concatenate([[0], np.cumsum([len(x) for x in batch])]).astype(np.int64)
    ahead = -1
    for hi, hay in enumerate(batch):
        state, base = 0, int(starts[hi])
        for pos, byte in enumerate(bytes(hay)):
            cl = cls[byte]
            if cl == 0:
                c["class0"] += 1
                state = 0
                continue
            e = None
            if state >= n_rows:
                if state < n_rows + n_single:
                    idx = state - n_rows
                    if idx < lds_n1:
                        c["single_lds"] += 1
                    elif state == ahead:
                        c["single_ahead"] += 1
                        ahead = -1
                    else:
                        c["single_global"] += 1
                        ahead = state + 1
                    x, y = chain[idx]
                    if (y >> 24) == cl:
                        e = x
                        c["single_answers"] += 1
                    else:
                        c["single_leans"] += 1
                else:
                    idx = state - n_rows - n_single
                    c["two_lds" if idx < lds_n2 else "two_global"] += 1
                    x, y, z, w = chain2[idx]
                    if (y >> 24) == cl:
                        e = x
                        c["two_first"] += 1
                    elif (w >> 24) == cl:
                        e = z
                        c["two_second"] += 1
                    else:
                        c["two_leans"] += 1
                if e is None:
                    state = y & 0xFFFFFF
                    assert state < n_rows
            if e is None:
                if state < hot_rows and cl <= DFA_LDS_COLS:
                    c["lds_rows"] += 1
                elif cl <= hot_cols:
                    c["hot"] += 1
                else:
                    c["cold"] += 1
                    if state < hot_rows:
                        c["lds_row_col_above_32"] += 1
                e = hot[(state << hot_l2) + cl - 1] if cl <= hot_cols else nxt[(state << l2c) + cl]
                if cl <= hot_cols:
                    assert e == nxt[(state << l2c) + cl]
            state = e & 0x0FFFFFFF
            if e >> 28:
                bits = e >> 28
                vl = bits if bits < DFA_END_LOOK_UP else out_y[state]
                assert vl >= bits
                ends.append((hi, pos + 1)); end_values.append(vl); end_states.append(state); end_global.append(base + pos)
                if 14 <= vl <= 16:
                    unit_start = (base + pos) // chunk * chunk
                    if int(np.searchsorted(starts, unit_start, side="right")) - 1 != hi and unit_start < base:
                        seam_ends.append((hi, pos + 1, vl))
    groups = []
    g_of = np.asarray(end_global, dtype=np.int64) // (64 * chunk)
    st = np.asarray(end_states, dtype=np.int64)
    for g in range(int((starts[-1] + 64 * chunk - 1) // (64 * chunk))):
        s = np.unique(st[g_of == g])
        groups.append({"records": int((g_of == g).sum()), "alias_low": _alias_pairs(s % DFA_PLACE_SLOTS),
                       "alias_hash": _alias_pairs(((s * DFA_PLACE_MUL) & 0xFFFFFFFF) >> DFA_PLACE_SHIFT)})
    return {"tiers": c, "ends": ends, "end_values": end_values, "seam_ends": seam_ends, "groups": groups}


def dfa_header_preconditions(img):
    """What the image must be for the tier tests to say anything (asserted, never skipped): rows, records of both kinds and columns beyond every LDS share of both launch
    shapes, more states than k_dfa_place's 4-byte entries tell apart by their slot, a state with 16 values or more.  Returns the figures."""
    t = dfa_tables(img)
    h = t["header"]
    f = {"n_states": h["n_states"], "n_rows": h["n_rows"], "n_single": h["n_single"], "n_two": h["n_states"] - h["n_rows"] - h["n_single"],
         "log2_classes": h["log2_classes"], "hot_log2": h["hot_log2"], "rare_bytes": int((t["cls"] == 0xFF).sum()), "max_values": int(t["out"][:, 1].max())}
    assert f["n_rows"] >= 1100 and f["n_single"] >= 2200 and f["n_two"] >= 1100 and f["log2_classes"] >= 6 and f["n_states"] > 16384 and f["max_values"] >= 16, f
    return f


def dfa_census_floors(census):
    """The floors of tests/test_dfa_tiers_cpu.py on one census: every tier at least 200 steps, ends of 14, 15 and 16 values at least 4 times each, at least 2 of them past a
    haystack seam inside their unit."""
    for tier in DFA_TIERS:
        assert census["tiers"][tier] >= 200, (tier, census["tiers"])
    for vl in (14, 15, 16):
        assert census["end_values"].count(vl) >= 4, (vl, census["end_values"].count(vl))
    assert len(census["seam_ends"]) >= 2, census["seam_ends"]


def dfa_alias_groups(census):
    """The groups of at most DFA_SUPER_ROOM records (their tokens fit one superblock).  Each must alias at least 10 pairs of distinct end states in either cache form, and
    there must be 4 of them."""
    small = [g for g in census["groups"] if g["records"] <= DFA_SUPER_ROOM]
    assert len(small) >= 4, [g["records"] for g in census["groups"]]
    for g in small:
        assert g["alias_low"] >= 10 and g["alias_hash"] >= 10, census["groups"]
    return small

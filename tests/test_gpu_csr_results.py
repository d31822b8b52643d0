"""The conventions of the three CSR result handles (am_fragments, am_needle_matrix, am_spans; csrc/am_fold.h CsrResult) on inputs of a few bytes: sizes against the
host mirror, the lazily fetched host copies (never NULL, fetched once), which device pointers are NULL, and that a freed result gives back every device byte."""
import ctypes as C
import gc

import numpy as np
import pytest

import alfred_margaret_amd as am

pytestmark = pytest.mark.gpu

NEEDLES = ["a", "aa", ","]
INPUTS = {
    "no_haystacks": [],
    "empty_haystacks": ["", "", ""],
    "five": ["a,b", "", "aaa", ",", "xyz"],
}
# items of input "five", by hand: "," cuts "a,b" and "," in two; the (needle, count) pairs a:1 ,:1 | a:3 aa:2 | ,:1; every fold step a , | a a aa a aa | ,;
# leftmost-longest a , | aa a | ,
FIVE_ITEMS = {"fragments": 7, "matrix": 5, "spans_all": 8, "spans_leftmost_longest": 5}
# (device_offsets, device_data) non-NULL?  Without haystacks nothing is in HBM.  With haystacks the offsets are; the items are once there is one -- the Splitter
# has a fragment per empty haystack, a matrix or a span list of nothing has no array (and am_spans_device_data answers NULL whenever there are no spans).
IN_HBM = {
    ("fragments", "no_haystacks"): (False, False), ("fragments", "empty_haystacks"): (True, True), ("fragments", "five"): (True, True),
    ("matrix", "no_haystacks"): (False, False), ("matrix", "empty_haystacks"): (True, False), ("matrix", "five"): (True, True),
    ("spans_all", "no_haystacks"): (False, False), ("spans_all", "empty_haystacks"): (True, False), ("spans_all", "five"): (True, True),
    ("spans_leftmost_longest", "no_haystacks"): (False, False), ("spans_leftmost_longest", "empty_haystacks"): (True, False),
    ("spans_leftmost_longest", "five"): (True, True),
}


class Kind:
    """One result kind: call(batch) -> the raw handle, the accessors' prefix, the item dtype, mirror(texts) -> (offsets, items) from the host mirror."""

    def __init__(self, name):
        self.name = name
        lib = am.api.libam()
        if name == "fragments":
            self.sp = am.Splitter(",")
            self.prefix, self.dtype = "am_fragments", am.api.FRAGMENT_DTYPE
            self.call = lambda b: self.sp.split_fragments(b)
        elif name == "matrix":
            self.a = am.Automaton(NEEDLES)
            self.t = am.api.ValuesTable(self.a)
            self.prefix, self.dtype = "am_needle_matrix", am.api.NEEDLE_COUNT_DTYPE
            self.call = lambda b: self.t.count_matrix_batch(am.CASE_SENSITIVE, b, raw=True)
        else:
            self.a = am.Automaton(NEEDLES)
            self.t = am.api.SpanTable(self.a)
            self.mode = am.api.SPANS_ALL if name == "spans_all" else am.api.SPANS_LEFTMOST_LONGEST
            self.prefix, self.dtype = "am_spans", am.api.SPAN_DTYPE
            self.call = lambda b: self.t.spans_batch(am.CASE_SENSITIVE, b, self.mode, raw=True)
        self.fn = lambda what: getattr(lib, self.prefix + "_" + what)

    def mirror(self, texts):
        if not texts:
            return np.zeros(1, np.uint64), np.zeros(0, self.dtype)
        if self.name == "fragments":
            lists = self.sp.split_batch(texts)
            offs = np.zeros(len(texts) + 1, np.uint64)
            offs[1:] = np.cumsum([len(x) for x in lists])
            frags = np.zeros(int(offs[-1]), self.dtype)
            k = 0
            for t, parts in zip(texts, lists):
                at = 0
                for p in parts:                              # (the fragments of a text in order, one separator byte between them)
                    frags[k] = (at, len(p))
                    at += len(p) + 1
                    k += 1
            return offs, frags
        if self.name == "matrix":
            return self.a.count_matrix_host_mirror(am.CASE_SENSITIVE, texts)
        return self.a.spans_host_mirror(am.CASE_SENSITIVE, texts, leftmost_longest=self.name == "spans_leftmost_longest")


def device_bytes():
    gc.collect()
    lib = am.api.libam()
    am.api.check(lib.am_release_device_memory())
    return int(lib.am_debug_device_buffer_bytes())


@pytest.mark.parametrize("input_name", sorted(INPUTS))
@pytest.mark.parametrize("kind_name", sorted(FIVE_ITEMS))
def test_csr_result_handle(kind_name, input_name):
    lib = am.api.libam()
    kind, texts = Kind(kind_name), INPUTS[input_name]
    exp_offs, exp_items = kind.mirror(texts)
    if input_name == "five":
        assert len(exp_items) == FIVE_ITEMS[kind_name]
    s = am.api._Slices(texts)
    b = C.c_void_p()
    am.api.check(lib.am_batch_upload(s.arr, s.n, C.byref(b)))
    try:
        kind.fn("free")(kind.call(b))                        # (the batch's own workspaces are sized by its first scan)
        before = device_bytes()
        x = kind.call(b)
        n, n_hay = int(kind.fn("size")(x)), int(kind.fn("haystacks")(x))
        assert (n, n_hay) == (len(exp_items), len(texts))
        po, pd = kind.fn("offsets")(x), kind.fn("data")(x)
        assert po and pd                                     # never NULL: a result without items answers with a placeholder element
        assert kind.fn("offsets")(x) == po and kind.fn("data")(x) == pd      # fetched once
        offs = np.frombuffer((C.c_char * ((n_hay + 1) * 8)).from_address(po), dtype=np.uint64)
        assert int(offs[0]) == 0 and int(offs[-1]) == n
        assert offs.tobytes() == exp_offs.tobytes()
        items = np.frombuffer((C.c_char * (n * kind.dtype.itemsize)).from_address(pd), dtype=kind.dtype) if n else np.zeros(0, kind.dtype)
        assert items.tobytes() == exp_items.tobytes()
        in_hbm = (bool(kind.fn("device_offsets")(x)), bool(kind.fn("device_data")(x)))
        assert in_hbm == IN_HBM[kind_name, input_name]
        kind.fn("free")(x)
        assert device_bytes() == before
    finally:
        lib.am_batch_destroy(b)

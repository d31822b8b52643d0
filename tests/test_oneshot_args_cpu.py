"""What a caller sees for bad arguments of the one-shot entry points that no other test pins: am_count, am_contains_any, am_run, am_split, am_count_by_needle and
am_count_matrix.  Every case is one call with one bad argument (or two, to pin which check wins) and asserts (return code, a word of am_last_error).  The expected
values were recorded from the library as it stood before the one-shot wrapper (csrc/am_fold.h with_oneshot_batch) replaced the entry points' own scaffolding; they
are a record, not a derivation.

Two columns: a box without a device, and one with.  am_count, am_contains_any and am_run look at the automaton's device before they look at the slices, so they
get a real automaton (the host-side build works anywhere); their slice-pointer, case_mode and out checks sit behind ensure_runtime() and read AM_ERR_NO_DEVICE
without a device.  The Splitter and the needle-id table cannot be made without a device: am_split and am_count_matrix get a fake non-null handle that no case here
lets them look at.  am_count_by_needle reads ids->n_needles between its slice check and its case_mode check: with a fake handle only the cases its null and slice
checks refuse can be called, and the invalid case_mode and the null counts_out are left to the column with a device, where the table is real."""
import ctypes as C

import numpy as np
import pytest

import alfred_margaret_amd as am

INVALID, NO_DEVICE = am.AM_ERR_INVALID, am.AM_ERR_NO_DEVICE
NO_DEV = (NO_DEVICE, b"no HIP device")
H, HAY, SLICE, CASE, OUT = "null_handle", "null_hay", "null_slice_ptr", "bad_case", "null_out"

# entry point -> {faults: (without a device, with a device)}; None: not called there
EXPECTED = {
    "am_count": {
        (H,): ((INVALID, b"null automaton"),) * 2,
        (HAY,): ((INVALID, b"hay is null"),) * 2,
        (SLICE,): (NO_DEV, (INVALID, b"slice with null ptr")),
        (CASE,): (NO_DEV, (INVALID, b"bad case_mode")),
        (OUT,): ((INVALID, b"counts_out is null"),) * 2,
        (H, HAY): ((INVALID, b"null automaton"),) * 2,
        (H, OUT): ((INVALID, b"counts_out is null"),) * 2,
        (HAY, OUT): ((INVALID, b"counts_out is null"),) * 2,
        (SLICE, CASE): (NO_DEV, (INVALID, b"slice with null ptr")),
    },
    "am_contains_any": {
        (H,): ((INVALID, b"null automaton"),) * 2,
        (HAY,): ((INVALID, b"hay is null"),) * 2,
        (SLICE,): (NO_DEV, (INVALID, b"slice with null ptr")),
        (CASE,): (NO_DEV, (INVALID, b"bad case_mode")),
        (OUT,): (NO_DEV, (INVALID, b"flags_out is null")),
        (H, HAY): ((INVALID, b"null automaton"),) * 2,
        (H, OUT): ((INVALID, b"null automaton"),) * 2,
        (HAY, OUT): ((INVALID, b"hay is null"),) * 2,
        (SLICE, CASE): (NO_DEV, (INVALID, b"slice with null ptr")),
    },
    "am_run": {
        (H,): ((INVALID, b"null automaton"),) * 2,
        (HAY,): ((INVALID, b"hay is null"),) * 2,
        (SLICE,): (NO_DEV, (INVALID, b"slice with null ptr")),
        (CASE,): (NO_DEV, (INVALID, b"bad case_mode")),
        (OUT,): (NO_DEV, (INVALID, b"out is null")),
        (H, HAY): ((INVALID, b"null automaton"),) * 2,
        (H, OUT): ((INVALID, b"null automaton"),) * 2,
        (HAY, OUT): ((INVALID, b"hay is null"),) * 2,
        (SLICE, CASE): (NO_DEV, (INVALID, b"slice with null ptr")),
    },
    "am_split": {
        (H,): ((INVALID, b"null splitter"),) * 2,
        (HAY,): ((INVALID, b"hay is null"),) * 2,
        (SLICE,): ((INVALID, b"slice with null ptr"),) * 2,
        (CASE,): ((INVALID, b"case_mode must be"),) * 2,
        (OUT,): ((INVALID, b"out is null"),) * 2,
        (H, HAY): ((INVALID, b"null splitter"),) * 2,
        (H, OUT): ((INVALID, b"out is null"),) * 2,
        (HAY, CASE): ((INVALID, b"hay is null"),) * 2,
        (SLICE, CASE): ((INVALID, b"slice with null ptr"),) * 2,
    },
    "am_count_by_needle": {
        (H,): ((INVALID, b"null needle ids"),) * 2,
        (HAY,): ((INVALID, b"hay is null"),) * 2,
        (SLICE,): ((INVALID, b"slice with null ptr"),) * 2,
        (CASE,): (None, (INVALID, b"case_mode must be")),
        (OUT,): (None, (INVALID, b"counts_out is null")),
        (H, HAY): ((INVALID, b"null needle ids"),) * 2,
        (H, OUT): ((INVALID, b"null needle ids"),) * 2,
        (HAY, CASE): ((INVALID, b"hay is null"),) * 2,
        (SLICE, OUT): ((INVALID, b"slice with null ptr"),) * 2,
        (CASE, OUT): (None, (INVALID, b"counts_out is null")),
    },
    "am_count_matrix": {
        (H,): ((INVALID, b"null needle ids"),) * 2,
        (HAY,): ((INVALID, b"hay is null"),) * 2,
        (SLICE,): ((INVALID, b"slice with null ptr"),) * 2,
        (CASE,): ((INVALID, b"case_mode must be"),) * 2,
        (OUT,): ((INVALID, b"out is null"),) * 2,
        (H, HAY): ((INVALID, b"null needle ids"),) * 2,
        (H, OUT): ((INVALID, b"out is null"),) * 2,
        (HAY, CASE): ((INVALID, b"hay is null"),) * 2,
        (SLICE, CASE): ((INVALID, b"slice with null ptr"),) * 2,
    },
}
CASES = [(name, faults) for name, table in EXPECTED.items() for faults in table]
RETURNS_A_HANDLE = ("am_run", "am_split", "am_count_matrix")


def gpu():
    import torch
    return torch.cuda.is_available()


class Handles:
    """What the calls are made with: a real automaton; without a device a fake Splitter and needle-id table that are never looked at, with one the real ones."""

    def __init__(self):
        self.automaton = am.Automaton(["he", "she"])
        self.splitter = self.table = None
        if gpu():
            self.splitter, self.table = am.Splitter(","), am.api.ValuesTable(self.automaton)

    def of(self, name):
        fake = C.c_void_p(1)
        if name in ("am_count", "am_contains_any", "am_run"):
            return self.automaton.device
        if name == "am_split":
            return self.splitter.device if self.splitter else fake
        return self.table.handle if self.table else fake


@pytest.fixture(scope="module")
def handles():
    return Handles()


def observe(handles, name, faults):
    """(return code, am_last_error) of one call of entry point `name` with the named faults, every other argument sound."""
    lib = am.api.libam()
    good = am.api._Slices(["she said"])
    bad = (am.api.Slice * 1)()
    bad[0].ptr, bad[0].off, bad[0].len = None, 0, 5
    result = C.c_void_p()
    out = C.byref(result) if name in RETURNS_A_HANDLE else np.zeros(8, np.uint64).ctypes.data
    rc = getattr(lib, name)(None if H in faults else handles.of(name), 2 if CASE in faults else 0,
                            None if HAY in faults else bad if SLICE in faults else good.arr, 1, None if OUT in faults else out)
    return rc, lib.am_last_error()


@pytest.mark.parametrize("name,faults", CASES, ids=["%s-%s" % (n, "+".join(f)) for n, f in CASES])
def test_bad_arguments_are_refused_as_recorded(handles, name, faults):
    expected = EXPECTED[name][faults][1 if gpu() else 0]
    if expected is None:
        return                                             # (not callable with a fake handle: see the module's docstring)
    rc, message = observe(handles, name, faults)
    print(name, faults, rc, message)
    assert rc == expected[0] and expected[1] in message, (rc, message, expected)

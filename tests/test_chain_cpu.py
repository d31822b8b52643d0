"""The chain selector (csrc/am_chain.h) and the owner search (csrc/am_rows.h) without a device: the per-element steps the kernels of am_chain.hip run -- the limited
walk, next[] for every element, the doubling rounds -- driven on the CPU over both chain views, against the sequential definition of the greedy selection, and
last_at_or_before against std::upper_bound; plain and under a sanitizer, in a stand-alone program."""
import os
import subprocess

from tests.conftest import ROOT


def _compile_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", *flags, "-I", os.path.join(ROOT, "alfred-margaret_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "chain_select_main.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)      # (a sanitizer's runtime is linked into the program: it starts in the environment as it is)
    assert out.returncode == 0 and "all checks passed" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_the_chain_selector_on_the_cpu_is_the_sequential_fold(tmp_path):
    """tests/native/chain_select_main.cpp: heads, the walk at limits 1, 2 and 32, chain_next for every element and doubling rounds until one marks nothing, over the
    Splitter's records and the spans' candidates: one chain through everything (n = 1 .. 70 and beyond 64 kept), two lengths, all heads, several rows whose relative
    starts begin again below the ends before them, n = 0; the rounds stay within ceil(log2(k)) + 1 for a kept path of k.  The owner search against std::upper_bound
    over ascending arrays with repeated values of 1, 2, 3, 64 and 65 entries, uint64_t with 64-bit and uint16_t with 32-bit indices."""
    _compile_and_run(tmp_path, "chain_select", [])


def test_the_chain_selector_under_a_sanitizer(tmp_path):
    """The same program with AddressSanitizer + UndefinedBehaviorSanitizer, their runtimes linked in statically: every array is a vector of exactly the size the
    device gives it.  A stand-alone program: no Python code runs under a sanitizer."""
    _compile_and_run(tmp_path, "chain_select_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"])

"""Match spans (am_spans*) next to the only other route to the same answer, on a BASELINE workload reduced to --gib GiB:

  (a)  am_spans_batch on a device-resident batch, AM_SPANS_ALL and AM_SPANS_LEFTMOST_LONGEST (the result stays in HBM: the raw handle);
  (b)  am_run_batch -> all records to the host (am_matches_data): the wire-bound part of the route without this fold, before any host fold;
  (b') amh_spans (am_run + the host mirror's sequential fold) on an eighth of the text, leftmost-longest: what the host fold adds to (b);
  (c)  am_count_batch: the scan alone, the ceiling.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed, the first haystacks' spans are held to the definition (tests/spans_reference.py over the oracle), both modes.
GiB/s are haystack bytes over the host clock around calls that end in a device synchronise (warm-up first, the median of --reps repetitions).  Kernel times come
from the library's HIP-event brackets (am_profile_*) in a pass of their own.  Workspace = the peak of am_debug_device_buffer_bytes over one call, sampled by a
thread, minus its value before.  Run on the MI355X box:
    python tests/measure/spans.py --workload natural_100k_10GiB --gib 2 --hay-kib 1024 --out spans_natural.md
"""
import argparse
import ctypes as C
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import alfred_margaret_amd as am                    # noqa: E402
from alfred_margaret_amd import synth               # noqa: E402

KERNELS = ("sf", "dfa", "dfa_place", "permute", "scan", "hidx", "spans_count", "spans_write", "spans_mark", "spans_rank", "spans_best", "spans_candidates", "spans_heads",
           "spans_walk", "spans_next", "spans_double", "spans_emit")


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def peak_buffer_bytes(lib, fn):
    """max of am_debug_device_buffer_bytes while fn() runs, above its value before"""
    before, peak, stop = int(lib.am_debug_device_buffer_bytes()), [0], threading.Event()

    def sample():
        while not stop.is_set():
            peak[0] = max(peak[0], int(lib.am_debug_device_buffer_bytes()))
            time.sleep(0.0002)

    th = threading.Thread(target=sample)
    th.start()
    try:
        fn()
    finally:
        stop.set()
        th.join()
    return max(peak[0] - before, 0)


def held_to_the_definition(a, t, case, needles, sample):
    """The spans of a few small haystacks against tests/spans_reference.py; returns how many were compared."""
    from oracle import oracle
    from tests import spans_reference as ref
    o = oracle.Machine(needles)
    n = 0
    for mode in (ref.ALL, ref.LEFTMOST_LONGEST):
        offs, spans = t.spans_texts(case, sample, mode)
        rows = ref.spans(o, case, mode, needles, sample)
        flat = [(s, ln, h, v) for h, r in enumerate(rows) for s, ln, v in r]
        assert offs.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist() and spans.tolist() == flat, ("the spans differ from the definition", mode)
        n += len(flat)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="natural_100k_10GiB")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--hay-kib", type=int, default=1024, help="haystack size in KiB (0: the workload's own)")
    ap.add_argument("--lines", action="store_true", help="the batch of the text's lines (split on '\\n' in HBM)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip (b'): no copy of the text in host memory")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    dev = torch.device("cuda:0")
    lib = am.api.libam()
    w = synth.WORKLOADS[args.workload]
    needles = synth.needles_for(args.workload)
    n_cells = int(args.gib * (1 << 20))
    hay_bytes = args.hay_kib * 1024 if args.hay_kib else int(w["hay_bytes"])
    n_hay = n_cells * 1024 // hay_bytes
    n_cells = n_hay * hay_bytes // 1024
    text, n_bytes = synth.haystacks_device(needles, w["mixed"], 0, n_cells, dev, natural=bool(w.get("natural")))
    offs = torch.arange(n_hay + 1, dtype=torch.int64, device=dev) * hay_bytes
    case = w["case"]
    a = am.Automaton(needles)
    t = am.SpanTable(a)
    docs = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), n_hay, n_bytes, C.byref(docs)))
    b, shape = docs, "%d haystacks of %d bytes" % (n_hay, hay_bytes)
    if args.lines:
        ends = (text[:n_bytes - 1] == ord(".")) & (text[1:n_bytes] == ord(" "))      # synth's text has no line ends of its own: the blank after every full stop becomes one
        text[1:n_bytes][ends] = ord("\n")
        del ends
        torch.cuda.synchronize()
        b, doc_offs = am.Splitter("\n").lines_batch(docs)
        shape = "%d lines (%.1f bytes on average)" % (int(doc_offs[-1]), n_bytes / max(int(doc_offs[-1]), 1))
    gib = n_bytes / float(1 << 30)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, %d needles, case %d" % (args.workload, gib, shape, len(needles), case))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    head = text[:min(n_bytes, 4 * 16384)].cpu().numpy()
    compared = held_to_the_definition(a, t, case, needles, [bytes(head[i * 16384:(i + 1) * 16384]) for i in range(4)])
    say("held to the definition first: %d spans of the first 64 KiB, both modes, equal" % compared)
    say("")
    seen = {}

    split = {am.api.SPANS_ALL: [], am.api.SPANS_LEFTMOST_LONGEST: []}      # (seconds in the call, seconds in am_spans_free) of every run

    def run_a(mode):
        t0 = time.perf_counter()
        x = t.spans_batch(case, b, mode, raw=True)
        t1 = time.perf_counter()
        seen[mode] = (int(lib.am_spans_size(x)), int(lib.am_spans_rounds(x)))
        lib.am_spans_free(x)
        split[mode].append((t1 - t0, time.perf_counter() - t1))

    rows = []
    t_all, _ = timed(lambda: run_a(am.api.SPANS_ALL), args.reps)
    rows.append(("(a) am_spans_batch, AM_SPANS_ALL, device-resident", t_all))
    t_ll, _ = timed(lambda: run_a(am.api.SPANS_LEFTMOST_LONGEST), args.reps)
    rows.append(("(a) am_spans_batch, AM_SPANS_LEFTMOST_LONGEST, device-resident", t_ll))
    for mode, name in ((am.api.SPANS_ALL, "AM_SPANS_ALL"), (am.api.SPANS_LEFTMOST_LONGEST, "AM_SPANS_LEFTMOST_LONGEST")):
        calls, frees = zip(*split[mode][1:])                # (without the warm-up)
        rows.append(("    %s: the call alone / am_spans_free alone: %.1f / %.1f ms" % (name, np.median(calls) * 1e3, np.median(frees) * 1e3), float(np.median(calls))))
    parts = {"run": [], "copy": []}
    n_records = 0
    for rep in range(1 + min(args.reps, 3)):
        m = C.c_void_p()
        t0 = time.perf_counter()
        am.api.check(lib.am_run_batch(a.device, case, b, C.byref(m)))
        t1 = time.perf_counter()
        n_records = int(lib.am_matches_size(m))
        p = lib.am_matches_data(m)
        assert p or not n_records
        t2 = time.perf_counter()
        lib.am_matches_free(m)
        if rep:
            parts["run"].append(t1 - t0); parts["copy"].append(t2 - t1)
    tb = {k: float(np.median(v)) for k, v in parts.items()}
    rows.append(("(b) am_run_batch + %.2f GB of records to the host (no host fold yet)" % (n_records * 16 / 1e9), tb["run"] + tb["copy"]))
    rows.append(("    (b) am_run_batch alone (records stay in HBM)", tb["run"]))
    n_rows = int(doc_offs[-1]) if args.lines else n_hay
    counts = np.zeros(max(n_rows, 1), np.uint64)
    total = C.c_uint64(0)
    tc, _ = timed(lambda: am.api.check(lib.am_count_batch(a.device, case, b, counts.ctypes.data, C.byref(total))), args.reps)
    rows.append(("(c) am_count_batch (the scan alone)", tc))
    say("| what | ms | GiB/s of scanned text |")
    say("|---|---|---|")
    for name, sec in rows:
        say("| %s | %.1f | %.1f |" % (name, sec * 1e3, gib / sec if sec > 0 else float("nan")))
    if not args.no_host and not args.lines:
        k = max(n_hay // 8, 1)
        host_text = text[:k * hay_bytes].cpu().numpy()
        slices = [host_text[i * hay_bytes:(i + 1) * hay_bytes] for i in range(k)]
        t0 = time.perf_counter()
        _, sp = a.spans_host_mirror(case, slices, leftmost_longest=True)
        th = time.perf_counter() - t0
        say("| (b') amh_spans, leftmost-longest, on %d haystacks (an eighth): am_run + records to the host + the host fold, %d spans | %.1f | %.1f |" % (
            k, len(sp), th * 1e3, (k * hay_bytes / float(1 << 30)) / th))
    say("")
    n_all, n_ll = seen[am.api.SPANS_ALL][0], seen[am.api.SPANS_LEFTMOST_LONGEST][0]
    say("leftmost-longest / (b) = %.2f x, all / (b) = %.2f x; %d records, %d values (%.2f per record), %d spans kept (%.1f MB against %.1f MB of records), %d doubling rounds" % (
        (tb["run"] + tb["copy"]) / t_ll, (tb["run"] + tb["copy"]) / t_all, n_records, n_all, n_all / max(n_records, 1), n_ll, n_ll * 24 / 1e6, n_records * 16 / 1e6,
        seen[am.api.SPANS_LEFTMOST_LONGEST][1]))
    say("")
    for mode, name in ((am.api.SPANS_ALL, "AM_SPANS_ALL"), (am.api.SPANS_LEFTMOST_LONGEST, "AM_SPANS_LEFTMOST_LONGEST")):
        say("peak of the library's device buffers during one %s call, records, result and workspace: %.1f MB" % (name, peak_buffer_bytes(lib, lambda: run_a(mode)) / 1e6))
    am.api.check(lib.am_profile_enable(1))
    for mode, name in ((am.api.SPANS_ALL, "AM_SPANS_ALL"), (am.api.SPANS_LEFTMOST_LONGEST, "AM_SPANS_LEFTMOST_LONGEST")):
        am.api.check(lib.am_profile_reset())
        run_a(mode)
        say("")
        say("kernels of one am_spans_batch, %s (HIP events): " % name + ", ".join("%s %.2f ms x %d" % (k, ms, n) for k, ms, n in (_prof(lib, k) for k in KERNELS) if n))
    lib.am_profile_enable(0)
    say("")
    if args.lines:
        lib.am_batch_destroy(b)
    lib.am_batch_destroy(docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _prof(lib, key):
    ms, n = C.c_double(0), C.c_uint64(0)
    lib.am_profile_read(key.encode(), C.byref(ms), C.byref(n))
    return key, float(ms.value), int(n.value)


if __name__ == "__main__":
    main()

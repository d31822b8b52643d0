"""Coordinates (am_coords_create, am_coords_spans, am_coords_ranges) on a BASELINE workload reduced to --gib GiB, leftmost-longest spans of the workload's whole
dictionary, next to what they are compared with:

  index    am_coords_create (coords_tiles and one coords_scan per class) for code points alone and for all three classes, by the host clock and by the library's
           HIP-event brackets (am_profile_*), against a device-to-device copy of the same text (torch, which calls hipMemcpyDtoD) in the same run: the ratio;
  stages   am_coords_spans (code points, UTF-16) and am_coords_ranges (code points) over an am_spans* made once, by the host clock and by the brackets;
  host     the route they replace: the same spans copied to the host (am_spans_data on a fresh copy of the result: 24 bytes per span), before any host decoding,
           alternating with index + stage;
  search   with --lines the same text as a batch of its lines: every line start is the haystack's base, so coords_ranges there against coords_ranges on the
           documents is the price of the searched line start.

Existing calls against the parent commit: tests/measure/extract.py --root <the parent's checkout> (am_spans_batch, am_extract_batch), as the templates change did.
Before anything is timed the first 64 KiB are held to the definition (tests/coords_reference.py over the oracle's spans).
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum; --once runs
every call exactly once and nothing else, for a run under `rocprofv3 --kernel-trace --stats -- python tests/measure/coords.py ... --once`.  Run on the MI355X box:
    python tests/measure/coords.py --workload natural_100k_10GiB --gib 2 --out coords_docs.md
    python tests/measure/coords.py --workload natural_100k_10GiB --gib 2 --lines --out coords_lines.md
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="natural_100k_10GiB")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--hay-kib", type=int, default=1024, help="haystack size in KiB (0: the workload's own)")
    ap.add_argument("--lines", action="store_true", help="the batch of the text's lines (split on '\\n' in HBM)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="every call once, nothing else: for a run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-host", action="store_true", help="skip the copy of the spans to the host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, HERE)
    import alfred_margaret_amd as am
    from alfred_margaret_amd import synth
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
    ends = (text[:n_bytes - 1] == ord(".")) & (text[1:n_bytes] == ord(" "))      # synth's text has no line ends of its own: the blank after every full stop becomes one
    text[1:n_bytes][ends] = ord("\n")
    del ends
    offs = torch.arange(n_hay + 1, dtype=torch.int64, device=dev) * hay_bytes
    torch.cuda.synchronize()
    case = w["case"]
    docs = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), n_hay, n_bytes, C.byref(docs)))
    b, shape = docs, "%d haystacks of %d bytes" % (n_hay, hay_bytes)
    if args.lines:
        b, doc_offs = am.Splitter("\n").lines_batch(docs)
        shape = "%d lines (%.1f bytes on average)" % (int(doc_offs[-1]), n_bytes / max(int(doc_offs[-1]), 1))
    total = int(lib.am_batch_total_bytes(b))
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    def prof(key):
        ms, n = C.c_double(0), C.c_uint64(0)
        lib.am_profile_read(key.encode(), C.byref(ms), C.byref(n))
        return float(ms.value)

    def kernels(fn, keys):
        am.api.check(lib.am_profile_enable(1))
        am.api.check(lib.am_profile_reset())
        try:
            fn()
            return {k: prof(k) for k in keys}
        finally:
            lib.am_profile_enable(0)

    def row(name, t, note=""):
        say("| %s | %.1f | %.1f .. %.1f | %s |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, note))

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, case %d, %d needles, leftmost-longest spans" % (args.workload, total / float(1 << 30), shape, case, len(needles)))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    a = am.Automaton(needles)
    t = am.api.SpanTable(a)
    LL = am.api.SPANS_LEFTMOST_LONGEST

    # held to the definition first
    from oracle import oracle
    from tests import coords_reference as cref, spans_reference as sref
    head = text[:min(n_bytes, 4 * 16384)].cpu().numpy()
    sample = [bytes(head[i * 2048:(i + 1) * 2048]) for i in range(32)]
    rows = sref.spans(oracle.Machine(needles), case, sref.LEFTMOST_LONGEST, needles, sample)
    for unit in (am.CODE_POINTS, am.UTF16):
        offs_s, spans_s, ranges_s = a.locate(case, sample, unit=unit)
        want = [(cref.span(h, s, n, unit), cref.span_range(h, s, n, unit)) for h, r in zip(sample, rows) for s, n, _ in r]
        got = [((int(s["start"]), int(s["len"])), tuple(int(v) for v in r)) for s, r in zip(spans_s, ranges_s)]
        assert got == want, ("locate differs from the definition", unit)
    say("held to the definition first: the first 64 KiB as 32 haystacks, spans and ranges in code points and UTF-16: equal")
    say("")

    state = {}
    sp = t.spans_batch(case, b, LL, raw=True)
    n_span = int(lib.am_spans_size(sp))

    def index(lines, utf16):
        state["c"] = None                                   # (the previous index is freed first: one index in HBM at a time)
        state["c"] = am.Coords(b, lines=lines, utf16=utf16)

    def conv(unit):
        lib.am_spans_free(state["c"].spans(sp, unit, raw=True))

    def ranges(unit):
        lib.am_ranges_free(state["c"].ranges(sp, unit, raw=True))

    copy_dst = torch.empty(total, dtype=torch.uint8, device=dev)
    src_view = text[:total] if not args.lines else torch.empty(total, dtype=torch.uint8, device=dev)

    def dtod():
        copy_dst.copy_(src_view)
        torch.cuda.synchronize()

    def spans_to_host():
        fresh = state["c"].spans(sp, am.BYTES, raw=True)    # a plain copy of the result in HBM: its host copy has not been made
        t0 = time.perf_counter()
        p = lib.am_spans_data(fresh)
        dt = time.perf_counter() - t0
        assert p
        lib.am_spans_free(fresh)
        return dt

    if args.once:
        index(True, True)
        conv(am.CODE_POINTS)
        conv(am.UTF16)
        ranges(am.CODE_POINTS)
        say("every call once (for a kernel trace)")
    else:
        say("| what | ms (median of %d) | min .. max | |" % args.reps)
        say("|---|---|---|---|")
        t_copy = timed(dtod, args.reps)
        row("device-to-device copy of the text", t_copy, "%.2f GB read and written" % (total / 1e9))
        t_cp = timed(lambda: index(False, False), args.reps)
        row("am_coords_create, code points", t_cp, "%.2f x the copy; index %.1f MB" % (t_cp[0] / t_copy[0], state["c"].index_bytes / 1e6))
        t_all = timed(lambda: index(True, True), args.reps)
        row("am_coords_create, code points + UTF-16 + lines", t_all, "%.2f x the copy; index %.1f MB = %.1f %% of the text" % (
            t_all[0] / t_copy[0], state["c"].index_bytes / 1e6, 100.0 * state["c"].index_bytes / max(total, 1)))
        t_s1 = timed(lambda: conv(am.CODE_POINTS), args.reps)
        row("am_coords_spans, code points", t_s1, "%d spans, %.2f GB as am_span" % (n_span, n_span * 24 / 1e9))
        t_s2 = timed(lambda: conv(am.UTF16), args.reps)
        row("am_coords_spans, UTF-16", t_s2)
        t_r = timed(lambda: ranges(am.CODE_POINTS), args.reps)
        row("am_coords_ranges, code points", t_r, "%.2f GB as am_span_range" % (n_span * 32 / 1e9))
        kk = kernels(lambda: (index(True, True), conv(am.CODE_POINTS), conv(am.UTF16), ranges(am.CODE_POINTS)), ("coords_tiles", "coords_scan", "coords_spans", "coords_ranges"))
        say("")
        say("kernels (HIP events, one run): coords_tiles %.3f ms = %.2f TB/s of text read, coords_scan %.3f ms (three sums), coords_spans %.3f ms (code points + UTF-16), "
            "coords_ranges %.3f ms" % (kk["coords_tiles"], total / (kk["coords_tiles"] * 1e-3) / 1e12 if kk["coords_tiles"] else float("nan"), kk["coords_scan"], kk["coords_spans"],
                                       kk["coords_ranges"]))
        if not args.no_host:
            host, devr = [], []
            for _ in range(args.reps):                      # alternating: the wire, then the device route (index + spans + ranges)
                host.append(spans_to_host())
                t0 = time.perf_counter()
                index(True, False)
                conv(am.CODE_POINTS)
                ranges(am.CODE_POINTS)
                devr.append(time.perf_counter() - t0)
            th, td = float(np.median(host)), float(np.median(devr))
            say("")
            say("the spans to the host (am_spans_data, %.2f GB, before any host decoding), alternating with index (code points + lines) + am_coords_spans + am_coords_ranges: "
                "%.1f ms (%.1f .. %.1f) against %.1f ms (%.1f .. %.1f) = %.1f x" % (n_span * 24 / 1e9, th * 1e3, min(host) * 1e3, max(host) * 1e3, td * 1e3, min(devr) * 1e3,
                                                                                    max(devr) * 1e3, th / td))
    say("")
    state["c"] = None
    lib.am_spans_free(sp)
    if args.lines:
        lib.am_batch_destroy(b)
    lib.am_batch_destroy(docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()

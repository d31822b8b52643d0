"""Extract (am_fragments_from_spans, am_extract_batch) on a BASELINE workload reduced to --gib GiB, leftmost-longest spans of the workload's whole dictionary with
--context code points either side, both modes, next to the wire-bound part of the route through the host:

  stage    am_fragments_from_spans alone over an am_spans* made once, AM_EXTRACT_EACH and AM_EXTRACT_MERGED, by the host clock;
  whole    am_extract_batch (am_spans_batch, the stage, am_batch_from_fragments), and its first and last part on their own;
  kernels  extract_windows, extract_heads, extract_emit and split_gather from the library's HIP-event brackets (am_profile_*) in a pass of their own -- or, with
           --once, every call exactly once and nothing else, for a run under `rocprofv3 --kernel-trace --stats -- python tests/measure/extract.py ... --once`;
           extract_windows as bytes of text TOUCHED over kernel time: every walk reads whole 16-byte groups, so a side of a window of w bytes of context touches
           between w and w + 15 bytes; the script counts, per fragment of AM_EXTRACT_EACH, round_up(len - span_len, 16) -- the two sides together, rounded up once;
  host     the same spans copied to the host (am_spans_data on a fresh result: 24 bytes per span), BEFORE any host work, alternating with the device route;
  parent   with --spans-only --root <tree> am_spans_batch and am_batch_from_fragments (over the Splitter's lines) on another checkout, e.g. the parent commit built in
           a directory of its own, for the same-session comparison.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed the first 64 KiB are held to the definition (tests/extract_reference.py over the oracle).
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum.  Run on the
MI355X box:
    python tests/measure/extract.py --workload natural_100k_10GiB --gib 2 --lines --out extract_lines.md
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
    ap.add_argument("--context", type=int, default=32, help="code points before and after every span")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--root", default=HERE, help="the checkout whose library is measured")
    ap.add_argument("--spans-only", action="store_true", help="am_spans_batch and am_batch_from_fragments only (runs on a checkout without extract)")
    ap.add_argument("--once", action="store_true", help="every call once, nothing else: for a run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-host", action="store_true", help="skip the copy of the spans to the host")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, os.path.abspath(args.root))
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
    offs = torch.arange(n_hay + 1, dtype=torch.int64, device=dev) * hay_bytes
    case = w["case"]
    docs = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), n_hay, n_bytes, C.byref(docs)))
    b, shape = docs, "%d haystacks of %d bytes" % (n_hay, hay_bytes)
    splitter = am.Splitter("\n")
    if args.lines:
        ends = (text[:n_bytes - 1] == ord(".")) & (text[1:n_bytes] == ord(" "))      # synth's text has no line ends of its own: the blank after every full stop becomes one
        text[1:n_bytes][ends] = ord("\n")
        del ends
        torch.cuda.synchronize()
        b, doc_offs = splitter.lines_batch(docs)
        shape = "%d lines (%.1f bytes on average)" % (int(doc_offs[-1]), n_bytes / max(int(doc_offs[-1]), 1))
    total = int(lib.am_batch_total_bytes(b))
    gib = total / float(1 << 30)
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    def prof(key):
        ms, n = C.c_double(0), C.c_uint64(0)
        lib.am_profile_read(key.encode(), C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def kernels(fn, keys):
        am.api.check(lib.am_profile_enable(1))
        am.api.check(lib.am_profile_reset())
        try:
            fn()
            return {k: prof(k)[0] for k in keys}
        finally:
            lib.am_profile_enable(0)

    def row(name, t, note=""):
        say("| %s | %.1f | %.1f .. %.1f | %s |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, note))

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, case %d, %d needles, leftmost-longest spans, %d code points of context%s" % (
        args.workload, gib, shape, case, len(needles), args.context, " -- checkout %s" % args.root if args.spans_only else ""))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    a = am.Automaton(needles)
    t = am.api.SpanTable(a)
    LL = am.api.SPANS_LEFTMOST_LONGEST
    state = {}

    def spans_only():
        if state.get("sp"):
            lib.am_spans_free(state["sp"])
        state["sp"] = t.spans_batch(case, b, LL, raw=True)

    if args.spans_only:
        say("| what | ms (median of %d) | min .. max | |" % args.reps)
        say("|---|---|---|---|")
        row("am_spans_batch, leftmost-longest", timed(spans_only, args.reps), "%d spans" % int(lib.am_spans_size(state["sp"])))
        lib.am_spans_free(state.pop("sp"))
        fr = splitter.split_fragments(docs)                # (the lines of the documents: with --lines they need the text's line ends, which it has by now)
        row("am_batch_from_fragments over the lines of the documents", timed(lambda: lib.am_batch_destroy(_from_fragments(am, lib, docs, fr)), args.reps),
            "%d fragments" % int(lib.am_fragments_size(fr)))
        lib.am_fragments_free(fr)
    else:
        sys.path.insert(0, HERE)
        from oracle import oracle
        from tests import extract_reference as xref, spans_reference as sref
        head = text[:min(total, 4 * 16384)].cpu().numpy()
        sample = [bytes(head[i * 2048:(i + 1) * 2048]) for i in range(32)]
        o = oracle.Machine(needles)
        for merged in (False, True):
            got = a.extract(case, sample, args.context, args.context, merged=merged)
            want = xref.extract(o, case, sref.LEFTMOST_LONGEST, needles, sample, args.context, args.context, xref.MERGED if merged else xref.EACH)
            rows = []
            for i in range(len(sample)):
                rows.append(want[2][want[0][i]:want[0][i + 1]])
            assert got == rows, ("extract differs from the definition", merged)
        say("held to the definition first: the first 64 KiB as 32 haystacks, both modes: equal")
        say("")
        B = A = args.context

        def stage(merged):
            if state.get("fr"):
                lib.am_fragments_free(state["fr"])
            state["fr"] = t.fragments_from_spans(b, state["sp"], B, A, merged, raw=True)

        def gather():
            lib.am_batch_destroy(_from_fragments(am, lib, b, state["fr"]))

        def whole(merged):
            nb, fr = C.c_void_p(), C.c_void_p()
            am.api.check(lib.am_extract_batch(t.handle, case, LL, B, A, int(merged), b, C.byref(nb), C.byref(fr)))
            state["new_total"] = int(lib.am_batch_total_bytes(nb))
            lib.am_batch_destroy(nb)
            lib.am_fragments_free(fr)

        def spans_to_host():
            sp = t.spans_batch(case, b, LL, raw=True)
            t0 = time.perf_counter()
            p = lib.am_spans_data(sp)
            dt = time.perf_counter() - t0
            assert p
            lib.am_spans_free(sp)
            return dt

        if args.once:
            spans_only()
            for merged in (False, True):
                stage(merged)
                gather()
            say("every call once (for a kernel trace)")
        else:
            say("| what | ms (median of %d) | min .. max | |" % args.reps)
            say("|---|---|---|---|")
            t_spans = timed(spans_only, args.reps)
            n_span = int(lib.am_spans_size(state["sp"]))
            row("am_spans_batch, leftmost-longest", t_spans, "%d spans, %.2f GB as am_span" % (n_span, n_span * 24 / 1e9))
            res = {}
            for merged in (False, True):
                name = "AM_EXTRACT_MERGED" if merged else "AM_EXTRACT_EACH"
                t_stage = timed(lambda: stage(merged), args.reps)
                n_frag = int(lib.am_fragments_size(state["fr"]))
                t_gather = timed(gather, args.reps)
                t_whole = timed(lambda: whole(merged), args.reps)
                row("am_fragments_from_spans, %s" % name, t_stage, "%d fragments" % n_frag)
                row("am_batch_from_fragments over them", t_gather, "%.2f GB of snippets" % (state["new_total"] / 1e9))
                row("am_extract_batch, %s" % name, t_whole)
                res[merged] = (t_stage, t_gather, t_whole, n_frag, state["new_total"])
            # bytes of text the walks touch, from the fragments of AM_EXTRACT_EACH: per fragment round_up(len - span_len, 16)
            stage(False)
            touched = _touched(torch, lib, state["fr"], state["sp"], n_span)
            for merged in (False, True):
                kk = kernels(lambda: (stage(merged), gather()), ("extract_windows", "extract_heads", "extract_emit", "split_gather"))
                say("")
                say("%s kernels (HIP events, one run): extract_windows %.3f ms = %.2f TB/s of text touched (%d bytes: per span its context rounded up to whole 16-byte groups), "
                    "extract_heads %.3f ms, extract_emit %.3f ms, split_gather %.3f ms = %.2f TB/s of snippets (read + written)" % (
                        "AM_EXTRACT_MERGED" if merged else "AM_EXTRACT_EACH", kk["extract_windows"], touched / (kk["extract_windows"] * 1e-3) / 1e12 if kk["extract_windows"] else float("nan"),
                        touched, kk["extract_heads"], kk["extract_emit"], kk["split_gather"],
                        2 * res[merged][4] / (kk["split_gather"] * 1e-3) / 1e12 if kk["split_gather"] else float("nan")))
            if not args.no_host:
                host, devr = [], []
                for _ in range(args.reps):                  # alternating: the wire, then the device route
                    host.append(spans_to_host())
                    t0 = time.perf_counter()
                    whole(False)
                    devr.append(time.perf_counter() - t0)
                th, td = float(np.median(host)), float(np.median(devr))
                say("")
                say("the spans to the host (am_spans_data, %.2f GB, before any host work), alternating with am_extract_batch AM_EXTRACT_EACH: %.1f ms (%.1f .. %.1f) against %.1f ms (%.1f .. %.1f) "
                    "= %.1f x" % (n_span * 24 / 1e9, th * 1e3, min(host) * 1e3, max(host) * 1e3, td * 1e3, min(devr) * 1e3, max(devr) * 1e3, th / td))
                say("the same copy against the stage alone (am_fragments_from_spans): %.1f ms against %.1f ms = %.1f x" % (th * 1e3, res[False][0][0] * 1e3, th / res[False][0][0]))
        for k in ("fr",):
            if state.get(k):
                lib.am_fragments_free(state.pop(k))
        if state.get("sp"):
            lib.am_spans_free(state.pop("sp"))
    say("")
    if args.lines:
        lib.am_batch_destroy(b)
    lib.am_batch_destroy(docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out_lines) + "\n")


def _from_fragments(am, lib, src, fr):
    nb = C.c_void_p()
    am.api.check(lib.am_batch_from_fragments(src, fr, C.byref(nb)))
    return nb


def _touched(torch, lib, fr, sp, n_span):
    """Sum over the fragments of AM_EXTRACT_EACH of round_up(fragment len - span len, 16), on the device."""
    if n_span == 0:
        return 0
    f = _device_view(torch, lib.am_fragments_device_data(fr), n_span * 2)
    s = _device_view(torch, lib.am_spans_device_data(sp), n_span * 3)
    ctx = f.view(n_span, 2)[:, 1] - s.view(n_span, 3)[:, 1]
    return int((((ctx + 15) // 16) * 16).sum().item())


def _device_view(torch, ptr, n_words):
    """int64[n_words] over device memory the library owns (no copy)."""
    class _Iface:
        pass
    x = _Iface()
    x.__cuda_array_interface__ = {"shape": (n_words,), "typestr": "<i8", "data": (int(ptr), False), "version": 3}
    return torch.as_tensor(x, device="cuda:0")


if __name__ == "__main__":
    main()

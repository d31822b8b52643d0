"""Whole-word matching (am_span_table_create_words, am_count_spans_by_needle*) on a BASELINE workload reduced to --gib GiB, next to the plain tables and to the only
other route to the same answer:

  share   of the AM_SPANS_ALL rows the default class keeps;
  plain   am_spans_batch with a table without a class, both span modes (--plain-only --root <tree>: the same on another checkout, e.g. the parent commit built in a
          directory of its own, for the same-session comparison: the plain instantiations must not have moved);
  words   am_spans_batch with the default class, both span modes, spans_count and spans_write beside their plain times (under IgnoreCase the count pass walks
          backwards as well: this prices the second walk);
  counts  am_count_spans_by_needle_batch against am_count_by_needle_batch: call time and histogram kernel time;
  host    am_spans_batch (plain, AM_SPANS_ALL) + the spans to the host (am_spans_data), before any host filter: the wire-bound part of the host route to whole-word
          term counts.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed the first 64 KiB are held to the definition (tests/words_reference.py over the oracle): spans in both modes and the counts.
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum (the
run-to-run spread).  Kernel times come from the library's HIP-event brackets (am_profile_*) in a pass of their own.  Run on the MI355X box:
    python tests/measure/words.py --workload natural_100k_10GiB --gib 2 --hay-kib 1024 --out words_natural.md
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
    ap.add_argument("--root", default=HERE, help="the checkout whose library is measured")
    ap.add_argument("--plain-only", action="store_true", help="tables without a class only (runs on a checkout without whole-word matching)")
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
    a = am.Automaton(needles)
    plain = am.SpanTable(a)
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

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, %d needles, case %d%s" % (args.workload, gib, shape, len(needles), case, " -- checkout %s" % args.root if args.plain_only else ""))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    modes = ((am.api.SPANS_ALL, "AM_SPANS_ALL"), (am.api.SPANS_LEFTMOST_LONGEST, "AM_SPANS_LEFTMOST_LONGEST"))
    sizes = {}

    def spans_call(table, mode, key):
        def run():
            x = table.spans_batch(case, b, mode, raw=True)
            sizes[key, mode] = int(lib.am_spans_size(x))
            lib.am_spans_free(x)
        return run

    def row(name, t):
        say("| %s | %.1f | %.1f .. %.1f | %.1f |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, gib / t[0] if t[0] > 0 else float("nan")))

    words = None
    if not args.plain_only:
        sys.path.insert(0, HERE)
        from oracle import oracle
        from tests import words_reference as wref
        words = am.SpanTable(a, word_bytes=True)
        head = text[:min(n_bytes, 4 * 16384)].cpu().numpy()
        sample = [bytes(head[i * 16384:(i + 1) * 16384]) for i in range(4)]
        o = oracle.Machine(needles)
        compared = 0
        for mode, _ in modes:
            got_offs, got = words.spans_texts(case, sample, mode)
            rows = wref.spans(o, case, mode, needles, sample, wref.DEFAULT_CLASS)
            flat = [(s, ln, h, v) for h, r in enumerate(rows) for s, ln, v in r]
            assert got_offs.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist() and got.tolist() == flat, ("the whole-word spans differ from the definition", mode)
            compared += len(flat)
        assert words.count_by_needle_texts(case, sample).tolist() == wref.counts(o, case, needles, sample, wref.DEFAULT_CLASS), "the whole-word counts differ from the definition"
        say("held to the definition first: %d whole-word spans of the first 64 KiB, both modes, and the %d term counts: equal" % (compared, len(needles)))
        say("")

    say("| what | ms (median of %d) | min .. max | GiB/s of scanned text |" % args.reps)
    say("|---|---|---|---|")
    for mode, name in modes:
        row("plain table, am_spans_batch, %s" % name, timed(spans_call(plain, mode, "plain"), args.reps))
    kp = kernels(spans_call(plain, am.api.SPANS_ALL, "plain"), ("spans_count", "spans_write"))
    if words is not None:
        for mode, name in modes:
            row("whole-word table, am_spans_batch, %s" % name, timed(spans_call(words, mode, "words"), args.reps))
        kw = kernels(spans_call(words, am.api.SPANS_ALL, "words"), ("spans_count", "spans_write"))
        values = am.ValuesTable(a)
        t_plain_counts = timed(lambda: values.count_by_needle_batch(case, b), args.reps)
        t_word_counts = timed(lambda: words.count_by_needle_batch(case, b), args.reps)
        row("am_count_by_needle_batch (every match)", t_plain_counts)
        row("am_count_spans_by_needle_batch (whole words)", t_word_counts)
        k_plain = kernels(lambda: values.count_by_needle_batch(case, b), ("needle_hist",))
        k_words = kernels(lambda: words.count_by_needle_batch(case, b), ("needle_hist_words",))

        def host_route():
            x = plain.spans_batch(case, b, am.api.SPANS_ALL, raw=True)
            try:
                assert lib.am_spans_data(x) or not lib.am_spans_size(x)
            finally:
                lib.am_spans_free(x)

        t_host = timed(host_route, min(args.reps, 3))
        row("host route: plain am_spans_batch AM_SPANS_ALL + %.2f GB of spans to the host (no host filter yet)" % (sizes["plain", am.api.SPANS_ALL] * 24 / 1e9), t_host)
    say("")
    say("kernels of one plain AM_SPANS_ALL call (HIP events): spans_count %.2f ms, spans_write %.2f ms; %d spans, %d leftmost-longest" % (
        kp["spans_count"], kp["spans_write"], sizes["plain", am.api.SPANS_ALL], sizes["plain", am.api.SPANS_LEFTMOST_LONGEST]))
    if words is not None:
        n_all, n_kept = sizes["plain", am.api.SPANS_ALL], sizes["words", am.api.SPANS_ALL]
        say("kernels of one whole-word AM_SPANS_ALL call (HIP events): spans_count %.2f ms, spans_write %.2f ms; %d spans, %d leftmost-longest" % (
            kw["spans_count"], kw["spans_write"], n_kept, sizes["words", am.api.SPANS_LEFTMOST_LONGEST]))
        say("share of spans kept by the default class: %d of %d = %.1f %%" % (n_kept, n_all, 100.0 * n_kept / max(n_all, 1)))
        say("histogram kernel (HIP events): needle_hist %.2f ms, needle_hist_words %.2f ms" % (k_plain["needle_hist"], k_words["needle_hist_words"]))
        say("whole-word term counts, device route / host route's wire-bound part: %.1f ms / %.1f ms = %.2f x" % (
            t_word_counts[0] * 1e3, t_host[0] * 1e3, t_host[0] / t_word_counts[0]))
    say("")
    if args.lines:
        lib.am_batch_destroy(b)
    lib.am_batch_destroy(docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

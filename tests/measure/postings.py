"""Postings (am_postings_batch, am_postings_from_spans) on a BASELINE workload reduced to --gib GiB, next to the route it replaces:

  yardstick  am_spans_batch(AM_SPANS_LEFTMOST_LONGEST) and am_spans_data: the spans of the batch copied to the host, 24 bytes each -- what a caller without the
             stage does BEFORE it sorts on the host -- and the same followed by np.argsort(kind="stable") of the needle column (once: it takes seconds);
  stage      am_postings_from_spans over the held spans: by the host clock, and kernel by kernel from the library's HIP-event brackets (am_profile_*) in a pass of
             its own -- post_keys, per pass post_hist / post_scan / post_scatter, post_gather, post_offsets, post_df; the (key, index) pairs a pass moves against a
             device-to-device copy of as many bytes;
  call       am_postings_batch by the host clock, and the stage's share of it;
  row        am_spans_of_needle for the most frequent needle.

--baseline: the yardstick alone, with nothing this stage added -- so that the same script runs over an older build of the library (--root: the tree to import).
--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed the first 64 KiB are held to the definition (tests/postings_reference.py over the oracle).
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum.  Run on the
MI355X box:
    python tests/measure/postings.py --workload natural_100k_10GiB --gib 2 --lines --out postings_lines.md
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ("post_keys", "post_hist", "post_scan", "post_scatter", "post_gather", "post_offsets", "post_df")


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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline", action="store_true", help="the yardstick alone: am_spans_batch, the copy, the host sort")
    ap.add_argument("--root", default=HERE, help="the tree whose alfred_margaret_amd is imported")
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
    if args.lines:
        ends = (text[:n_bytes - 1] == ord(".")) & (text[1:n_bytes] == ord(" "))      # synth's text has no line ends of its own: the blank after every full stop becomes one
        text[1:n_bytes][ends] = ord("\n")
        del ends
        torch.cuda.synchronize()
        b, doc_offs = am.Splitter("\n").lines_batch(docs)
        shape = "%d lines (%.1f bytes on average)" % (int(doc_offs[-1]), n_bytes / max(int(doc_offs[-1]), 1))
    total = int(lib.am_batch_total_bytes(b))
    gib = total / float(1 << 30)
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    def row(name, t, note=""):
        say("| %s | %.1f | %.1f .. %.1f | %.1f | %s |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, gib / t[0], note))

    def kernels_ms(fn):
        am.api.check(lib.am_profile_enable(1))
        am.api.check(lib.am_profile_reset())
        try:
            fn()
            out = {}
            for k in KERNELS:
                ms, n = C.c_double(0), C.c_uint64(0)
                lib.am_profile_read(k.encode(), C.byref(ms), C.byref(n))
                out[k] = (float(ms.value), int(n.value))
            return out
        finally:
            lib.am_profile_enable(0)

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, case %d%s" % (args.workload, gib, shape, case, " -- the yardstick alone" if args.baseline else ""))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    a = am.Automaton(needles)
    n_needles = len(needles)
    table = am.SpanTable(a)
    LL = am.api.SPANS_LEFTMOST_LONGEST
    say("| what | ms (median of %d) | min .. max | GiB/s of text | |" % args.reps)
    say("|---|---|---|---|---|")
    if not args.baseline:
        # held to the definition first
        from tests import postings_reference as ref
        head = text[:min(total, 4 * 16384)].cpu().numpy()
        sample = [bytes(head[i * 2048:(i + 1) * 2048]) for i in range(32)]
        rows = ref.rows_of(needles, case, sample, ref.LEFTMOST_LONGEST)
        data, source, df = ref.postings_sparse(rows)
        with table.postings_texts(case, sample, LL) as x:
            sp = x.spans
            got = list(zip(sp["start"].tolist(), sp["len"].tolist(), sp["haystack"].tolist(), sp["needle"].tolist()))
            assert got == data and x.source.tolist() == source, "the postings differ from the definition"
            gf = x.doc_freq
            assert {int(v): int(gf[v]) for v in np.flatnonzero(gf)} == df, "the document frequencies differ from the definition"
            assert np.array_equal(x.offsets, np.searchsorted(sp["needle"], np.arange(n_needles + 1), side="left").astype(np.uint64))
        say("| held to the definition first: the first 64 KiB as 32 haystacks, %d postings of %d needles: equal | | | | |" % (len(data), len(df)))
    # the yardstick: the spans, their copy to the host, the host's stable sort
    state = {}

    def spans():
        if state.get("s"):
            lib.am_spans_free(state["s"])
        state["s"] = table.spans_batch(case, b, LL, raw=True)

    for turn in (1, 2):                                     # (twice: the spread between the two is what "unchanged" means)
        t_spans = timed(spans, args.reps)
        n_span = int(lib.am_spans_size(state["s"]))
        row("am_spans_batch, leftmost-longest, turn %d" % turn, t_spans, "%d spans" % n_span)
    state["copy"] = []
    for _ in range(args.reps + 1):
        spans()                                             # (a result copies once: a fresh one per repetition)
        t0 = time.perf_counter()
        p = lib.am_spans_data(state["s"])
        assert p
        state["copy"].append(time.perf_counter() - t0)
    cp = state["copy"][1:]
    t_copy = (float(np.median(cp)), float(min(cp)), float(max(cp)))
    row("am_spans_data: the %d spans (%d bytes) to the host -- the yardstick" % (n_span, n_span * 24), t_copy)
    host = np.frombuffer((C.c_char * (n_span * 24)).from_address(p), dtype=am.api.SPAN_DTYPE) if n_span else np.zeros(0, am.api.SPAN_DTYPE)
    t0 = time.perf_counter()
    perm = np.argsort(host["needle"], kind="stable")
    t_sort = time.perf_counter() - t0
    t0 = time.perf_counter()
    sorted_rows = host[perm]
    t_take = time.perf_counter() - t0
    del perm, sorted_rows, host
    say("| np.argsort(kind=\"stable\") of the needle column on the host, once | %.1f | | | then the rows taken in that order: %.1f ms; the copy and both: **%.1f ms** |" % (
        t_sort * 1e3, t_take * 1e3, (t_copy[0] + t_sort + t_take) * 1e3))
    if not args.baseline:
        spans()

        def stage():
            state["x"] = table.postings_from_spans(state["s"])

        t_stage = timed(stage, args.reps)
        k = kernels_ms(stage)
        k_all = sum(v[0] for v in k.values())
        passes = am.api.postings_geometry(n_needles)[2]
        row("am_postings_from_spans", t_stage, "%d passes over %d needles; kernels by their HIP events (ms, launches): %s = %.2f ms = **%.3f x** the copy of the spans" % (
            passes, n_needles, ", ".join("%s %.2f (%d)" % (name[5:], k[name][0], k[name][1]) for name in KERNELS), k_all, k_all / (t_copy[0] * 1e3)))
        # the pairs a pass moves: 8 bytes per span read and written -- against a device-to-device copy of as many bytes
        pairs = torch.empty(max(n_span, 1) * 8, dtype=torch.uint8, device=dev)
        other = torch.empty_like(pairs)

        def d2d():
            other.copy_(pairs)
            torch.cuda.synchronize()

        t_d2d = timed(d2d, args.reps)
        per_pass = (k["post_hist"][0] + k["post_scan"][0] + k["post_scatter"][0]) / max(passes, 1)
        row("a device-to-device copy of the pairs of one pass (%d bytes)" % (n_span * 8), t_d2d, "one pass (hist + scan + scatter) takes %.2f ms = %.1f x this copy" % (
            per_pass, per_pass / (t_d2d[0] * 1e3)))
        del pairs, other

        def call():
            state["x"] = table.postings_batch(case, b, LL)

        t_call = timed(call, args.reps)
        row("am_postings_batch", t_call, "the stage (host clock) is %.0f %% of the call; the call = **%.3f x** am_spans_batch + the copy + the host sort" % (
            100.0 * t_stage[0] / t_call[0], t_call[0] / (t_spans[0] + t_copy[0] + t_sort + t_take)))
        x = state["x"]
        df = x.doc_freq
        top = int(np.argmax(np.diff(x.offsets)))

        def one_row():
            lib.am_spans_free(x.spans_of(top, raw=True))

        t_row = timed(one_row, args.reps)
        row("am_spans_of_needle, the most frequent needle", t_row, "%d of %d postings, in %d of %d haystacks; %d needles occur at all" % (
            int(np.diff(x.offsets)[top]), x.size, int(df[top]), x.n_hay, int(np.count_nonzero(df))))
        state.pop("x")
        del x
    say("")
    lib.am_spans_free(state["s"])
    if args.lines:
        lib.am_batch_destroy(b)
    lib.am_batch_destroy(docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()

"""Proximity (am_near_batch, am_near_spans) on a BASELINE workload reduced to --gib GiB, next to the route it replaces:

  yardstick  am_spans_batch(AM_SPANS_LEFTMOST_LONGEST) and am_spans_data: the spans of the batch copied to the host, 24 bytes each -- what a caller without the
             stage does BEFORE any join on the host (the join itself and the upload of its flags are not timed);
  stage      am_near_spans over the held spans with 1 and with 64 queries over random group masks: by the host clock, and kernel by kernel from the library's
             HIP-event brackets (am_profile_*) in a pass of its own -- near_bits, near_words, near_count, near_place (the exclusive sum), near_emit;
  call       am_near_batch by the host clock, and the stage's share of it;
  select     am_select_near + am_batch_from_selection for query 0.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed the first 64 KiB are held to the definition (tests/near_reference.py over the oracle).
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum.  Run on the
MI355X box:
    python tests/measure/near.py --workload natural_100k_10GiB --gib 2 --lines --out near_lines.md
"""
import argparse
import ctypes as C
import os
import random
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ("near_bits", "near_words", "near_count", "near_place", "near_emit")


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
    ap.add_argument("--max-gap", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, HERE)
    import alfred_margaret_amd as am
    from alfred_margaret_amd import synth
    import torch
    from tests import near_reference as ref

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
                out[k] = float(ms.value)
            return out
        finally:
            lib.am_profile_enable(0)

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, case %d" % (args.workload, gib, shape, case))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    a = am.Automaton(needles)
    n = len(needles)
    table = am.SpanTable(a)
    rng = random.Random(11)
    masks = [0 if rng.random() < 0.25 else rng.getrandbits(32) & rng.getrandbits(32) & rng.getrandbits(32) | (1 << rng.randrange(32)) for _ in range(n)]
    queries = [(rng.randrange(32), rng.randrange(32), args.max_gap, q % 4 == 3) for q in range(64)]
    # held to the definition first
    head = text[:min(total, 4 * 16384)].cpu().numpy()
    sample = [bytes(head[i * 2048:(i + 1) * 2048]) for i in range(32)]
    x = am.Near(table, masks, queries).near_texts(case, sample)
    offsets, pairs, fired, counts = ref.near(ref.rows_of(needles, case, sample), masks, queries)
    assert x.offsets.tolist() == offsets and [tuple(int(v) for v in p) for p in x.pairs.tolist()] == pairs and x.counts.tolist() == counts, "the pairs differ from the definition"
    say("| what | ms (median of %d) | min .. max | GiB/s of text | |" % args.reps)
    say("|---|---|---|---|---|")
    say("| held to the definition first: the first 64 KiB as 32 haystacks, 64 queries, %d pairs: equal | | | | |" % len(pairs))
    del x
    # the yardstick: the spans, and their copy to the host
    state = {}

    def spans():
        if state.get("s"):
            lib.am_spans_free(state["s"])
        state["s"] = table.spans_batch(case, b, am.api.SPANS_LEFTMOST_LONGEST, raw=True)

    t_spans = timed(spans, args.reps)
    n_span = int(lib.am_spans_size(state["s"]))
    row("am_spans_batch, leftmost-longest", t_spans, "%d spans" % n_span)

    def copy():
        spans()                                             # (a result copies once: a fresh one per repetition, its own time taken off below)
        t0 = time.perf_counter()
        assert lib.am_spans_data(state["s"])
        state["copy"].append(time.perf_counter() - t0)

    state["copy"] = []
    for _ in range(args.reps + 1):
        copy()
    cp = state["copy"][1:]
    t_copy = (float(np.median(cp)), float(min(cp)), float(max(cp)))
    row("am_spans_data: the %d spans (%d bytes) to the host -- the yardstick" % (n_span, n_span * 24), t_copy)
    spans()
    for nq in (1, 64):
        near = am.Near(table, masks, queries[:nq])

        def stage():
            state["x"] = near.near_spans(state["s"])

        t_stage = timed(stage, args.reps)
        k = kernels_ms(stage)
        k_all = sum(k.values())
        n_pairs = int(lib.am_near_hits_size(state["x"].handle))
        row("am_near_spans, %d quer%s" % (nq, "y" if nq == 1 else "ies"), t_stage, "%d pairs; kernels by their HIP events: %s = %.2f ms = **%.3f x** the copy of the spans" % (
            n_pairs, ", ".join("%s %.2f" % (name[5:], k[name]) for name in KERNELS), k_all, k_all / (t_copy[0] * 1e3)))

        def call():
            state["x"] = near.near_batch(case, b)

        t_call = timed(call, args.reps)
        row("am_near_batch, %d quer%s" % (nq, "y" if nq == 1 else "ies"), t_call, "the stage (host clock) is %.0f %% of the call; the call = %.2f x am_spans_batch + the copy" % (
            100.0 * t_stage[0] / t_call[0], t_call[0] / (t_spans[0] + t_copy[0])))

        def select():
            nb = state["x"].select(0, batch=b).batch(b)
            lib.am_batch_destroy(nb)

        t_sel = timed(select, args.reps)
        kept = state["x"].select(0, batch=b).size
        row("am_select_near + am_batch_from_selection, query 0 of %d" % nq, t_sel, "%d haystacks kept" % kept)
        state.pop("x")
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

"""Per-needle exact case (am_span_table_create_cased, csrc/am_cased.h) on a BASELINE workload reduced to --gib GiB, with spellings on 0 %, 10 % and 100 % of the
handles (a spelling is the needle capitalised, or in capitals), next to the plain table, the whole-word table and the route the feature replaces:

  share   of the AM_SPANS_ALL rows each table keeps;
  spans   am_spans_batch, both span modes, per table;
  counts  am_count_spans_by_needle_batch per table (the plain table: am_count_by_needle_batch's kernel);
  host    plain am_spans_batch (AM_SPANS_ALL) + the spans to the host (am_spans_data), before any host filter: the wire-bound part of "scan with AM_IGNORE_CASE and
          filter on the host".

--base-only --root <tree>: the plain and the whole-word table only, on another checkout (the parent commit built in a directory of its own): run it several times
interleaved with this commit's --base-only; the parent's own run-to-run spread is the margin a difference has to leave.
--once: every call once and nothing timed, for a counter-free `rocprofv3 --kernel-trace --stats` run of its own, which gives the kernel times.
Before anything is timed the first 64 KiB are held to the definition (tests/cased_reference.py over the oracle).  Times are the host clock around calls that end in a
device synchronise: a warm-up, then the median of --reps repetitions with their minimum and maximum.  Run on the MI355X box:
    python tests/measure/exact_case.py --workload natural_100k_10GiB --gib 2 --hay-kib 1024 --out exact_case.md
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


def spellings(needles, percent):
    """Every (100 / percent)-th handle gets a spelling: capitalised, or -- every other one of those -- in capitals.  A needle without a cased letter gets none."""
    out = [None] * len(needles)
    if percent == 0:
        return out
    step = 100 // percent
    for k, v in enumerate(range(0, len(needles), step)):
        n = needles[v] if isinstance(needles[v], str) else needles[v].decode("utf-8")
        s = n.upper() if k % 2 else n[:1].upper() + n[1:]
        if s != n and len(s) == len(n):
            out[v] = s
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="natural_100k_10GiB")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--hay-kib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--root", default=HERE, help="the checkout whose library is measured")
    ap.add_argument("--base-only", action="store_true", help="the plain and the whole-word table only (runs on a checkout without exact case)")
    ap.add_argument("--once", action="store_true", help="every call once, nothing timed: for a kernel trace")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    sys.path.insert(0, os.path.abspath(args.root))
    import alfred_margaret_amd as am
    from alfred_margaret_amd import synth
    import torch

    dev = torch.device("cuda:0")
    lib = am.api.libam()
    w = synth.WORKLOADS[args.workload]
    needles = [n.lower() for n in synth.needles_for(args.workload)]
    hay_bytes = args.hay_kib * 1024
    n_hay = int(args.gib * (1 << 20)) * 1024 // hay_bytes
    n_cells = n_hay * hay_bytes // 1024
    text, n_bytes = synth.haystacks_device(needles, w["mixed"], 0, n_cells, dev, natural=bool(w.get("natural")))
    offs = torch.arange(n_hay + 1, dtype=torch.int64, device=dev) * hay_bytes
    a = am.Automaton(needles)
    b = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), n_hay, n_bytes, C.byref(b)))
    gib = n_bytes / float(1 << 30)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tables = [("plain", am.SpanTable(a)), ("whole words", am.SpanTable(a, word_bytes=True))]
    if not args.base_only:
        sys.path.insert(0, HERE)
        from oracle import oracle
        from tests import cased_reference as cref
        head = text[:min(n_bytes, 4 * 16384)].cpu().numpy()
        sample = [bytes(head[i * 16384:(i + 1) * 16384]) for i in range(4)]
        o = oracle.Machine(needles)
        for percent in (0, 10, 100):
            exact = spellings(needles, percent)
            t = am.SpanTable(a, exact=exact)
            tables.append(("exact on %d %% (%d spellings)" % (percent, sum(x is not None for x in exact)), t))
            if percent:
                for mode in (0, 1):
                    got_offs, got = t.spans_texts(1, sample, mode)
                    rows = cref.spans(o, 1, mode, needles, sample, exact)
                    flat = [(s, ln, h, v) for h, r in enumerate(rows) for s, ln, v in r]
                    assert got_offs.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist() and got.tolist() == flat, ("the spans differ from the definition", percent, mode)
        tables.append(("exact on 100 % + whole words", am.SpanTable(a, word_bytes=True, exact=spellings(needles, 100))))

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %d haystacks of %d bytes, %d lower-cased needles, AM_IGNORE_CASE -- checkout %s" % (
        args.workload, gib, n_hay, hay_bytes, len(needles), os.path.basename(os.path.abspath(args.root)) if args.base_only else "this commit"))
    say("")
    say("%s, %d CUs%s" % (info["arch"], info["n_cu"], "" if args.base_only else "; the first 64 KiB held to the definition first, both modes, 10 % and 100 %: equal"))
    say("")
    sizes = {}

    def spans_call(name, table, mode, fetch=False):
        def run():
            x = table.spans_batch(1, b, mode, raw=True)
            sizes[name, mode] = int(lib.am_spans_size(x))
            try:
                assert not fetch or lib.am_spans_data(x) or not lib.am_spans_size(x)
            finally:
                lib.am_spans_free(x)
        return run

    calls = []
    for name, t in tables:
        calls.append(("%s: am_spans_batch, AM_SPANS_ALL" % name, spans_call(name, t, 0)))
        calls.append(("%s: am_spans_batch, AM_SPANS_LEFTMOST_LONGEST" % name, spans_call(name, t, 1)))
        calls.append(("%s: am_count_spans_by_needle_batch" % name, lambda t=t: t.count_by_needle_batch(1, b)))
    if not args.base_only:
        calls.append(("host route: plain am_spans_batch AM_SPANS_ALL + the spans to the host (no host filter yet)", spans_call("host", tables[0][1], 0, fetch=True)))
    if args.once:
        for name, fn in calls:
            fn()
        say("every call made once")
    else:
        say("| what | ms (median of %d) | min .. max | GiB/s of scanned text |" % args.reps)
        say("|---|---|---|---|")
        for name, fn in calls:
            t = timed(fn, args.reps if not name.startswith("host route") else min(args.reps, 3))
            say("| %s | %.1f | %.1f .. %.1f | %.1f |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, gib / t[0] if t[0] > 0 else float("nan")))
    say("")
    n_all = sizes["plain", 0]
    for name, _ in tables:
        say("rows kept, %s: %d of %d = %.1f %% (%d leftmost-longest)" % (name, sizes[name, 0], n_all, 100.0 * sizes[name, 0] / max(n_all, 1), sizes[name, 1]))
    say("the spans of the plain table on the wire: %.2f GB" % (n_all * 24 / 1e9))
    say("")
    lib.am_batch_destroy(b)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

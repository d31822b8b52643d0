"""Substitute templates on the device (am_subst_table_create_templates: k_subst_tpl_count / k_subst_tpl_pieces in front of the scans, the compaction and the gather of
am_batch_substitute) on a BASELINE workload reduced to --gib GiB, AM_IGNORE_CASE.  Two tables over the same span table and the same spans:

  template  [<b>, MATCH, </b>] for every needle: the text's own spelling wrapped -- what no fixed replacement gives under AM_IGNORE_CASE;
  plain     "[" + needle + "]", through am_subst_table_create and k_subst_pieces: the splice as it was.

For each: the splice stage alone (am_batch_substitute over a spans result that is already in HBM) and the whole am_substitute_batch call, and the kernels of one splice
singly.  Beside them am_spans_batch and the copy of the same spans to the host (am_spans_data, 24 bytes per span): what the route without templates -- spans to the
host, a splice in Python, a fresh upload -- begins with.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed, the first 64 KiB are substituted through both tables and held to the definition (tests/template_reference.py over the oracle).
Host-clock figures are around calls that end in a device synchronise: a warm-up first, then the median of --reps repetitions.  Kernel times come from the library's
HIP-event brackets (am_profile_*) in a pass of their own, ONE run each.  Run on the MI355X box:
    python tests/measure/templates.py --workload natural_100k_10GiB --gib 2 --hay-kib 1024 --out templates_natural.md
The plain splice on another build of the library (the parent commit's) is measured by tests/measure/substitute.py in that tree, in the same session.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import alfred_margaret_amd as am                    # noqa: E402
from alfred_margaret_amd import synth               # noqa: E402

KERNELS = ("subst_tpl_count", "subst_pieces", "subst_scan", "subst_compact", "subst_gather")


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def _prof(lib, key):
    ms, n = C.c_double(0), C.c_uint64(0)
    lib.am_profile_read(key.encode(), C.byref(ms), C.byref(n))
    return float(ms.value), int(n.value)


def held_to_the_definition(r, case, needles, templates, sample):
    from oracle import oracle
    from tests import template_reference as tref
    got = r.substitute_texts(case, sample)
    assert got == tref.substitute(oracle.Machine(needles), case, needles, sample, templates), "the substituted texts differ from the definition"
    return sum(map(len, got))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="natural_100k_10GiB")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--hay-kib", type=int, default=1024)
    ap.add_argument("--lines", action="store_true", help="the batch of the text's lines (split on '\\n' in HBM)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    dev = torch.device("cuda:0")
    lib = am.api.libam()
    w = synth.WORKLOADS[args.workload]
    needles = synth.needles_for(args.workload)
    hay_bytes = args.hay_kib * 1024
    n_hay = int(args.gib * (1 << 30)) // hay_bytes
    text, n_bytes = synth.haystacks_device(needles, w["mixed"], 0, n_hay * hay_bytes // 1024, dev, natural=bool(w.get("natural")))
    offs = torch.arange(n_hay + 1, dtype=torch.int64, device=dev) * hay_bytes
    case = am.IGNORE_CASE
    a = am.Automaton(needles)
    t = am.SpanTable(a)
    sets = {"template [<b>, MATCH, </b>]": [["<b>", am.MATCH, "</b>"]] * len(needles), "plain [needle]": ["[" + x + "]" for x in needles]}
    tables = {k: am.SubstTable(t, v) for k, v in sets.items()}
    assert [r.templates for r in tables.values()] == [True, False]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    docs = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), n_hay, n_bytes, C.byref(docs)))
    b, shape = docs, "%d haystacks of %d bytes" % (n_hay, hay_bytes)
    if args.lines:
        ends = (text[:n_bytes - 1] == ord(".")) & (text[1:n_bytes] == ord(" "))      # synth's text has no line ends of its own: the blank after every full stop becomes one
        text[1:n_bytes][ends] = ord("\n")
        del ends
        torch.cuda.synchronize()
        b, doc_offs = am.Splitter("\n").lines_batch(docs)
        n_lines = int(doc_offs[-1])
        shape = "%d lines (%.1f bytes on average)" % (n_lines, n_bytes / max(n_lines, 1))
    gib = n_bytes / float(1 << 30)
    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, %d needles, AM_IGNORE_CASE" % (args.workload, gib, shape, len(needles)))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    head = text[:min(n_bytes, 4 * 16384)].cpu().numpy()
    sample = [bytes(head[i * 16384:(i + 1) * 16384]) for i in range(4)]
    for name in sets:
        say("held to the definition first, %s: %d bytes of output from the first 64 KiB, equal" % (name, held_to_the_definition(tables[name], case, needles, sets[name], sample)))
    say("")

    def spans_call():
        x = t.spans_batch(case, b, am.api.SPANS_LEFTMOST_LONGEST, raw=True)
        lib.am_spans_free(x)

    t_spans = timed(spans_call, args.reps)
    spans = t.spans_batch(case, b, am.api.SPANS_LEFTMOST_LONGEST, raw=True)
    n_span = int(lib.am_spans_size(spans))
    copies = []
    for rep in range(args.reps + 1):                        # the host copy is made once per result: a fresh result per repetition, the copy alone on the clock
        x = t.spans_batch(case, b, am.api.SPANS_LEFTMOST_LONGEST, raw=True)
        t0 = time.perf_counter()
        assert lib.am_spans_data(x)
        copies.append(time.perf_counter() - t0)
        lib.am_spans_free(x)
    t_copy = float(np.median(copies[1:]))
    say("| what | ms | GiB/s of source text |")
    say("|---|---|---|")
    say("| am_spans_batch, AM_SPANS_LEFTMOST_LONGEST (%d spans) | %.1f | %.1f |" % (n_span, t_spans * 1e3, gib / t_spans))
    say("| am_spans_data: the same spans to the host, %.2f GB (the copy alone) | %.1f | %.1f |" % (n_span * 24 / 1e9, t_copy * 1e3, gib / t_copy))
    results = {}
    for name, r in tables.items():
        def splice_call():
            nb = r.splice(b, spans, raw=True)
            results[name] = int(lib.am_batch_total_bytes(nb))
            lib.am_batch_destroy(nb)

        def whole_call():
            lib.am_batch_destroy(r.substitute_batch(case, b, raw=True))

        t_splice = timed(splice_call, args.reps)
        t_whole = timed(whole_call, args.reps)
        say("| %s: am_batch_substitute, the splice alone (%.2f GB out) | %.1f | %.1f |" % (name, results[name] / 1e9, t_splice * 1e3, gib / t_splice))
        say("| %s: am_substitute_batch, spans + splice | %.1f | %.1f |" % (name, t_whole * 1e3, gib / t_whole))
        say("| %s: splice / spans-to-host copy = %.2f x; am_substitute_batch - am_spans_batch = %.1f ms | | |" % (name, t_splice / t_copy, (t_whole - t_spans) * 1e3))
    say("")
    for name, r in tables.items():
        am.api.check(lib.am_profile_enable(1))
        am.api.check(lib.am_profile_reset())
        nb = r.splice(b, spans, raw=True)
        lib.am_profile_enable(0)
        total = int(lib.am_batch_total_bytes(nb))
        lib.am_batch_destroy(nb)
        prof = {k: _prof(lib, k) for k in KERNELS}
        say("%s, kernels of one am_batch_substitute (HIP events, one run): " % name + ", ".join("%s %.2f ms" % (k, prof[k][0]) for k in KERNELS if prof[k][1]) +
            "; sum %.2f ms; subst_gather: %.2f GB written, as many read: %.2f TB/s" % (sum(v[0] for v in prof.values()), total / 1e9,
                                                                                    2 * total / prof["subst_gather"][0] / 1e9))
    say("")
    lib.am_spans_free(spans)
    if args.lines:
        lib.am_batch_destroy(b)
    lib.am_batch_destroy(docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

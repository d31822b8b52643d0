"""Scores (am_score_batch) on a BASELINE workload reduced to --gib GiB, next to the folds it is a sibling of and the routes to the same numbers that exist without it:

  score    am_score_batch with 1 and with 8 weight columns by the host clock, and the kernel time of k_score from the library's HIP-event brackets (am_profile_*) in a
           pass of its own;
  scan     am_count_batch: the scan alone, the ceiling of every fold over it;
  hist     am_count_by_needle_batch and its kernel k_needle_hist on the same records: the same expansion of a record through its value list, so the yardstick of
           the fold;
  route 1  am_count_matrix_batch and the copy of its entries to the host (the sparse matrix-vector product on the host is not timed);
  route 2  am_run_batch and the copy of its records to the host (the fold on the host is not timed);
  top-k    am_scores_top_k(k = 100) and am_select_score over one column, next to copying the column to the host and np.argpartition there;
  --fold-only  am_count_by_needle_batch alone -- with --root <tree> on another checkout, e.g. the parent commit built in a directory of its own, for the same-session
           comparison of a fold this change did not touch.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed the first 64 KiB are held to the definition (tests/score_reference.py over the oracle).
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum.  Run on the
MI355X box:
    python tests/measure/score.py --workload natural_100k_10GiB --gib 2 --lines --out score_lines.md
"""
import argparse
import ctypes as C
import os
import random
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--root", default=HERE, help="the checkout whose library is measured")
    ap.add_argument("--label", default="", help="what the heading calls the checkout, e.g. `parent`")
    ap.add_argument("--fold-only", action="store_true", help="am_count_by_needle_batch only (runs on a checkout without scores)")
    ap.add_argument("--no-routes", action="store_true", help="skip the matrix and the record routes")
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
    n_src = int(lib.am_batch_haystacks(b))
    total = int(lib.am_batch_total_bytes(b))
    gib = total / float(1 << 30)
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    def row(name, t, note=""):
        say("| %s | %.1f | %.1f .. %.1f | %.1f | %s |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, gib / t[0], note))

    def prof(key):
        ms, n = C.c_double(0), C.c_uint64(0)
        lib.am_profile_read(key.encode(), C.byref(ms), C.byref(n))
        return float(ms.value), int(n.value)

    def kernel_ms(key, fn):
        am.api.check(lib.am_profile_enable(1))
        am.api.check(lib.am_profile_reset())
        try:
            fn()
            return prof(key)
        finally:
            lib.am_profile_enable(0)

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, case %d%s" % (args.workload, gib, shape, case, " -- %s" % args.label if args.label else ""))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    a = am.Automaton(needles)
    n = len(needles)
    table = am.api.ValuesTable(a, n)
    counts = np.zeros(n, np.uint64)
    say("| what | ms (median of %d) | min .. max | GiB/s of text | |" % args.reps)
    say("|---|---|---|---|---|")
    fold = lambda: am.api.check(lib.am_count_by_needle_batch(table.handle, case, b, counts.ctypes.data))
    t_hist = timed(fold, args.reps)
    if args.fold_only:
        row("am_count_by_needle_batch", t_hist)
    else:
        sys.path.insert(0, HERE)
        from tests import score_reference as ref
        rng = random.Random(7)
        cols = [[rng.randint(-1000, 1000) for _ in range(n)] for _ in range(8)]
        head = text[:min(total, 4 * 16384)].cpu().numpy()
        sample = [bytes(head[i * 2048:(i + 1) * 2048]) for i in range(32)]
        assert np.array_equal(a.score(case, sample, cols), ref.expect(needles, None, n, case, cols, sample)), "the scores differ from the definition"
        say("| held to the definition first: the first 64 KiB as 32 haystacks, 8 columns: equal | | | | |")
        total_values = C.c_uint64(0)
        t_scan = timed(lambda: am.api.check(lib.am_count_batch(a.device, case, b, None, C.byref(total_values))), args.reps)
        row("am_count_batch: the scan alone, the ceiling", t_scan, "%d values" % int(total_values.value))
        k_hist = kernel_ms("needle_hist", fold)
        row("am_count_by_needle_batch", t_hist, "k_needle_hist by its HIP events: %.3f ms in %d launch(es)" % k_hist)
        state = {}
        k_score = {}
        for n_cols in (1, 8):
            wts = am.Weights(table, cols[:n_cols])

            def score():
                state["x"] = wts.score_batch(case, b)

            t = timed(score, args.reps)
            k_score[n_cols] = kernel_ms("score", score)
            row("am_score_batch, %d column%s" % (n_cols, "" if n_cols == 1 else "s"), t,
                "k_score by its HIP events: %.3f ms in %d launch(es) = %.2f x k_needle_hist; the call = %.2f x am_count_by_needle_batch" % (
                    k_score[n_cols][0], k_score[n_cols][1], k_score[n_cols][0] / k_hist[0] if k_hist[0] > 0 else float("nan"), t[0] / t_hist[0]))
            t_score = t
        x = state["x"]
        # top-k and the range select over column 0 of the 8-column result
        t_top = timed(lambda: x.top_k(100), args.reps)
        t_sel = timed(lambda: x.select(1, 2 ** 62, batch=b), args.reps)
        col_dev = torch.from_numpy(x.scores[0]).to(dev)       # the same column in HBM, as a caller without the top-k would hold it
        torch.cuda.synchronize()

        def host_route():
            h = col_dev.cpu().numpy()                          # the column crosses, then the selection on the host
            k = min(100, n_src)
            return np.argpartition(-h, k - 1)[:k] if n_src else h

        t_host = timed(host_route, args.reps)
        say("| am_scores_top_k(k = 100), 1 column of %d scores | %.2f | %.2f .. %.2f | | %.1f x the host route |" % (n_src, t_top[0] * 1e3, t_top[1] * 1e3, t_top[2] * 1e3, t_host[0] / t_top[0]))
        say("| am_select_score(1 <= score), the same column | %.2f | %.2f .. %.2f | | |" % (t_sel[0] * 1e3, t_sel[1] * 1e3, t_sel[2] * 1e3))
        say("| the column to the host + np.argpartition(k = 100) | %.2f | %.2f .. %.2f | | |" % (t_host[0] * 1e3, t_host[1] * 1e3, t_host[2] * 1e3))
        del col_dev
        state.clear()
        del x
        if not args.no_routes:
            mstate = {}

            def matrix():
                mstate["m"] = table.count_matrix_batch(case, b, raw=True)

            def wire():
                mstate["e"] = am.api.matrix_to_numpy(mstate["m"])[1].shape[0]

            try:
                t_mx = timed(matrix, 1, warmup=0)
                t_wire = timed(wire, 1, warmup=0)
                row("route 1: am_count_matrix_batch", t_mx)
                row("route 1: its %d entries (%d bytes) to the host" % (mstate["e"], mstate["e"] * 16), t_wire)
                say("| route 1 in all (the matrix-vector product on the host not counted) | %.1f | | %.1f | %.1f x am_score_batch with 8 columns |" % (
                    (t_mx[0] + t_wire[0]) * 1e3, gib / (t_mx[0] + t_wire[0]), (t_mx[0] + t_wire[0]) / t_score[0]))
            except am.AmError as e:
                say("| route 1: am_count_matrix_batch failed: %s | | | | |" % e)
            finally:
                if mstate.get("m"):
                    lib.am_needle_matrix_free(mstate["m"])
            rstate = {}

            def run():
                m = C.c_void_p()
                am.api.check(lib.am_run_batch(a.device, case, b, C.byref(m)))
                rstate["m"] = m

            def records():
                rstate["n"] = am.api.matches_to_numpy(rstate["m"]).shape[0]

            try:
                t_run = timed(run, 1, warmup=0)
                t_rec = timed(records, 1, warmup=0)
                row("route 2: am_run_batch", t_run)
                row("route 2: its %d records (%d bytes) to the host" % (rstate["n"], rstate["n"] * 16), t_rec)
                say("| route 2 in all (the fold on the host not counted) | %.1f | | %.1f | %.1f x am_score_batch with 8 columns |" % (
                    (t_run[0] + t_rec[0]) * 1e3, gib / (t_run[0] + t_rec[0]), (t_run[0] + t_rec[0]) / t_score[0]))
            except am.AmError as e:
                say("| route 2: am_run_batch failed: %s | | | | |" % e)
            finally:
                if rstate.get("m"):
                    lib.am_matches_free(rstate["m"])
    say("")
    if args.lines:
        lib.am_batch_destroy(b)
    lib.am_batch_destroy(docs)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(out_lines) + "\n")


if __name__ == "__main__":
    main()

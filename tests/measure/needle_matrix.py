"""The term-document matrix (am_count_matrix*) next to the only other route to the same answer, on a BASELINE workload reduced to --gib GiB:

  (a) am_count_matrix_batch on a device-resident batch (the result stays in HBM: the raw handle);
  (b) am_run_batch -> all records to the host (am_matches_data): the wire-bound part of the route without this fold, which still needs a host fold that (a) does not;
  (c) am_count_by_needle_batch: the same scan with the cheaper fold; no matrix can beat it;
  (d) am_count_matrix from host slices.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of the workload's size.
GiB/s are haystack bytes over the host clock around calls that end in a device synchronise (warm-up first, the median of --reps repetitions).  Kernel times come
from the library's HIP-event brackets (am_profile_*) in a pass of their own, or from `rocprofv3 --kernel-trace --stats -- python tests/measure/needle_matrix.py
--kernels-only`.  Workspace = the peak of am_debug_device_buffer_bytes over one call, sampled by a thread, minus its value before.  Run on the MI355X box:
    python tests/measure/needle_matrix.py --workload natural_100k_10GiB --gib 2 --hay-kib 1024 --out needle_matrix_natural.md
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="natural_100k_10GiB")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--hay-kib", type=int, default=0, help="haystack size in KiB (0: the workload's own)")
    ap.add_argument("--lines", action="store_true", help="the batch of the text's lines (split on '\\n' in HBM)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="only (a), three times: the run to put under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-host", action="store_true", help="skip (d): no copy of the text in host memory")
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
    t = am.ValuesTable(a)
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

    waves = am.api.resident_waves()
    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, %d needles, case %d" % (args.workload, gib, shape, len(needles), case))
    say("")
    say("%s, %d CUs, resident_waves_per_cu = %d (16-per-CU launch %.3f ms, 32-per-CU launch %.3f ms)" % (info["arch"], info["n_cu"], waves[0], waves[1], waves[2]))
    say("")
    seen = {}

    def run_a():
        x = t.count_matrix_batch(case, b, raw=True)
        seen["entries"], seen["rows"] = int(lib.am_needle_matrix_size(x)), int(lib.am_needle_matrix_haystacks(x))
        lib.am_needle_matrix_free(x)

    if args.kernels_only:
        for _ in range(3):
            run_a()
        print("entries", seen["entries"])
    else:
        rows = []
        ta, _ = timed(run_a, args.reps)
        rows.append(("(a) am_count_matrix_batch, device-resident", ta))
        tc, _ = timed(lambda: t.count_by_needle_batch(case, b), args.reps)
        rows.append(("(c) am_count_by_needle_batch (the cheaper fold)", tc))
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
        if not args.no_host and not args.lines:
            host_text = text[:n_bytes].cpu().numpy()
            s = am.api._Slices([host_text[i * hay_bytes:(i + 1) * hay_bytes] for i in range(n_hay)])

            def run_d():
                x = C.c_void_p()
                am.api.check(lib.am_count_matrix(t.handle, case, s.arr, s.n, C.byref(x)))
                assert int(lib.am_needle_matrix_size(x)) == seen["entries"]
                lib.am_needle_matrix_free(x)

            td, _ = timed(run_d, min(args.reps, 3))
            rows.append(("(d) am_count_matrix from host slices", td))
        say("| what | ms | GiB/s of scanned text |")
        say("|---|---|---|")
        for name, sec in rows:
            say("| %s | %.1f | %.1f |" % (name, sec * 1e3, gib / sec if sec > 0 else float("nan")))
        say("")
        say("(a) / (b) = %.2f x; %d records, %d rows, %d entries (%.2f per row), result %.1f MB" % (
            (tb["run"] + tb["copy"]) / ta, n_records, seen["rows"], seen["entries"], seen["entries"] / max(seen["rows"], 1), (seen["entries"] * 16 + seen["rows"] * 8) / 1e6))
        say("")
        say("peak of the library's device buffers during one (a), result and workspace: %.1f MB" % (peak_buffer_bytes(lib, run_a) / 1e6))
        am.api.check(lib.am_profile_enable(1))
        am.api.check(lib.am_profile_reset())
        run_a()
        say("")
        say("kernels of one am_count_matrix_batch (HIP events): " + ", ".join(
            "%s %.2f ms x %d" % (k, ms, n) for k, ms, n in (_prof(lib, k) for k in ("sf", "dfa", "dfa_place", "permute", "scan", "hidx", "mx_values", "mx_combine", "mx_scatter",
                                                                                   "mx_rows", "mx_rows_lds", "mx_rows_wide")) if n))
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

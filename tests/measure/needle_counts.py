"""Per-needle match counts (am_count_by_needle*) next to the only other route to the same vector, on a BASELINE workload reduced to --gib GiB:

  (a) am_count_by_needle_batch on a device-resident batch;
  (b) am_run_batch -> records to the host (am_matches_data) -> expansion through machineValues and np.bincount on the host;
  (c) am_count_batch (the scan alone: the ceiling);
  (d) am_count_by_needle from host slices, next to am_run from host slices.

GiB/s are haystack bytes over the host clock around calls that end in a device synchronise (warm-up first, the median of --reps repetitions).  Kernel times come
from the library's HIP-event brackets (am_profile_*) in a pass of their own, or from `rocprofv3 --kernel-trace --stats -- python tests/measure/needle_counts.py
--kernels-only`; the share of adds the LDS tables absorbed from the instrumented kernel (AM_HIST_TRACE), again in a pass of its own.  Run on the MI355X box:
    python tests/measure/needle_counts.py --workload natural_100k_10GiB --gib 2 --out needle_counts_natural.md
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


def timed(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="natural_100k_10GiB")
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="only (a), three times: the run to put under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--no-host", action="store_true", help="skip (b)'s host fold and (d): no copy of the text or the records in host memory")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    dev = torch.device("cuda:0")
    lib = am.api.libam()
    w = synth.WORKLOADS[args.workload]
    needles = synth.needles_for(args.workload)
    n_cells = int(args.gib * (1 << 20))
    hay_bytes = int(w["hay_bytes"])
    n_hay = n_cells * 1024 // hay_bytes
    n_cells = n_hay * hay_bytes // 1024
    text, n_bytes = synth.haystacks_device(needles, w["mixed"], 0, n_cells, dev, natural=bool(w.get("natural")))
    offs = torch.arange(n_hay + 1, dtype=torch.int64, device=dev) * hay_bytes
    case = w["case"]
    a = am.Automaton(needles)
    t = am.ValuesTable(a)
    b = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), n_hay, n_bytes, C.byref(b)))
    gib = n_bytes / float(1 << 30)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    waves = am.api.resident_waves()
    info = am.device_info()
    say("## %s reduced to %.2f GiB (%d haystacks of %d bytes), %d needles, case %d" % (args.workload, gib, n_hay, hay_bytes, len(needles), case))
    say("")
    say("%s, %d CUs, resident_waves_per_cu = %d (16-per-CU launch %.3f ms, 32-per-CU launch %.3f ms)" % (info["arch"], info["n_cu"], waves[0], waves[1], waves[2]))
    say("")

    counts = {}

    def run_a():
        counts["a"] = t.count_by_needle_batch(case, b)

    if args.kernels_only:
        for _ in range(3):
            run_a()
        print("sum", int(counts["a"].sum()))
        lib.am_batch_destroy(b)
        return

    total = C.c_uint64(0)

    def run_c():
        am.api.check(lib.am_count_batch(a.device, case, b, None, C.byref(total)))

    rows = []
    ta, _ = timed(run_a, args.reps)
    rows.append(("(a) am_count_by_needle_batch, device-resident", ta))
    tc, _ = timed(run_c, args.reps)
    rows.append(("(c) am_count_batch (ceiling)", tc))
    assert int(counts["a"].sum()) == int(total.value), (int(counts["a"].sum()), int(total.value))

    # (b) the parent's route: records in HBM, then over the wire, then the host's fold
    voff, vals = a.values_off(), a.values()
    per_state = np.diff(voff).astype(np.int64)
    parts = {"run": [], "copy": [], "fold": []}
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
        t3 = t2
        if not args.no_host and n_records:
            recs = np.frombuffer((C.c_char * (n_records * am.api.MATCH_DTYPE.itemsize)).from_address(p), dtype=am.api.MATCH_DTYPE)
            by_state = np.bincount(recs["state"], minlength=len(per_state))
            host = np.zeros(len(needles), np.int64)
            np.add.at(host, vals, np.repeat(by_state, per_state))
            t3 = time.perf_counter()
            assert np.array_equal(host.astype(np.uint64), counts["a"]), "device and host folds disagree"
        lib.am_matches_free(m)
        if rep:
            parts["run"].append(t1 - t0); parts["copy"].append(t2 - t1); parts["fold"].append(t3 - t2)
    tb = {k: float(np.median(v)) for k, v in parts.items()}
    rows.append(("(b) am_run_batch + records to the host%s" % ("" if args.no_host else " + host fold (np.bincount)"), tb["run"] + tb["copy"] + tb["fold"]))
    rows.append(("    (b) am_run_batch alone (records stay in HBM)", tb["run"]))
    rows.append(("    (b) am_matches_data: %.2f GB of records over the wire" % (n_records * 16 / 1e9), tb["copy"]))
    if not args.no_host:
        rows.append(("    (b) host expansion + np.bincount", tb["fold"]))

    if not args.no_host:
        host_text = text[:n_bytes].cpu().numpy()
        hays = [host_text[i * hay_bytes:(i + 1) * hay_bytes] for i in range(n_hay)]
        s = am.api._Slices(hays)
        out = np.zeros(len(needles), np.uint64)

        def run_d():
            am.api.check(lib.am_count_by_needle(t.handle, case, s.arr, s.n, out.ctypes.data))

        def run_d_run():
            m = C.c_void_p()
            am.api.check(lib.am_run(a.device, case, s.arr, s.n, C.byref(m)))
            lib.am_matches_free(m)

        td, _ = timed(run_d, min(args.reps, 3))
        assert np.array_equal(out, counts["a"])
        rows.append(("(d) am_count_by_needle from host slices", td))
        tr, _ = timed(run_d_run, min(args.reps, 3))
        rows.append(("(d') am_run from host slices (records to the host)", tr))

    say("| what | ms | GiB/s of scanned text |")
    say("|---|---|---|")
    for name, sec in rows:
        say("| %s | %.1f | %.1f |" % (name, sec * 1e3, gib / sec if sec > 0 else float("nan")))
    say("")
    say("%d records, %d values (%.3f values per record), %d of %d needles seen" % (n_records, int(total.value), int(total.value) / max(n_records, 1),
                                                                                 int((counts["a"] > 0).sum()), len(needles)))

    # kernel times of (a), HIP events around every launch (a pass of its own: the brackets are not in the timings above)
    am.api.check(lib.am_profile_enable(1))
    am.api.check(lib.am_profile_reset())
    run_a()
    say("")
    say("kernels of one am_count_by_needle_batch (HIP events): " + ", ".join(
        "%s %.2f ms x %d" % (k, ms, n) for k, ms, n in (_prof(lib, k) for k in ("sf", "dfa", "dfa_place", "permute", "scan", "hidx", "needle_hist")) if n))
    lib.am_profile_enable(0)

    # share of the adds the LDS tables absorbed (the instrumented instantiation; a pass of its own)
    am.debug_set("AM_HIST_TRACE", 1)
    am.api.hist_adds()
    run_a()
    in_lds, in_hbm, in_flush = am.api.hist_adds()
    am.debug_set("AM_HIST_TRACE", -1)
    adds = in_lds + in_hbm
    say("")
    say("adds: %d, of which %d (%.2f %%) were combined in LDS and %d (%.2f %%) went to HBM one by one; %d flush adds: %.1f x fewer global atomics than values"
        % (adds, in_lds, 100.0 * in_lds / max(adds, 1), in_hbm, 100.0 * in_hbm / max(adds, 1), in_flush, adds / max(in_hbm + in_flush, 1)))
    say("")
    lib.am_batch_destroy(b)
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

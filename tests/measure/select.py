"""Select (am_select_any_batch + am_batch_from_selection) on a BASELINE workload reduced to --gib GiB, next to the only other route to the same batch and to a plain
copy of the same number of bytes:

  shares  needle subsets of the workload's dictionary are tried (one containsAny scan each) and the three whose kept share lies nearest to 1 %, 50 % and 99 % are
          measured; the shares are recorded;
  select  the whole am_select_any_batch + am_batch_from_selection call by the host clock, the two halves on their own, and the kernel times of select_plan, select_emit
          and select_gather from the library's HIP-event brackets (am_profile_*) in a pass of their own; the gather's TB/s of text (kept bytes read and written once);
  host    the route without select: am_contains_any_batch (the flags to the host), the compaction of the texts on the host with numpy (the texts are there already:
          their copy to the host is not timed), the kept texts and their offsets up again and am_batch_from_device over them;
  copy    a device-to-device copy (hipMemcpyDtoD through torch) of the kept bytes;
  scan    am_contains_any_batch alone -- with --scan-only --root <tree> the same on another checkout, e.g. the parent commit built in a directory of its own, for the
          same-session comparison of the scan before and after its flags were left in HBM.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed the first 64 KiB are held to the definition (tests/select_reference.py over the oracle).
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum.  Run on the
MI355X box:
    python tests/measure/select.py --workload natural_100k_10GiB --gib 2 --lines --out select_lines.md
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
    ap.add_argument("--scan-only", action="store_true", help="am_contains_any_batch only (runs on a checkout without select)")
    ap.add_argument("--subsets", default="", help="needle counts to measure instead of searching the shares, e.g. 1,64,100000")
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
    n_src = int(lib.am_batch_haystacks(b)) if hasattr(lib, "am_batch_haystacks") else n_hay
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

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, case %d%s" % (args.workload, gib, shape, case, " -- checkout %s" % args.root if args.scan_only else ""))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    flags = np.zeros(max(n_src, 1), np.uint8)
    automata = {}

    def automaton(k):
        if k not in automata:
            automata[k] = am.Automaton(needles[:k])
        return automata[k]

    def share(k):
        am.api.check(lib.am_contains_any_batch(automaton(k).device, case, b, flags.ctypes.data))
        return float(flags[:n_src].mean())

    if args.subsets:
        picked = [(int(k), share(int(k))) for k in args.subsets.split(",")]
    else:
        tried, k = [], 1
        while k < len(needles):
            tried.append((k, share(k)))
            k *= 4
        tried.append((len(needles), share(len(needles))))
        say("kept share by needle subset (the first k needles of the dictionary): " + ", ".join("k = %d: %.1f %%" % (k, 100 * s) for k, s in tried))
        say("")
        picked = []
        for target in (0.01, 0.5, 0.99):
            best = min(tried, key=lambda ks: abs(ks[1] - target))
            if best not in picked:
                picked.append(best)

    def row(name, t, bytes_moved=None):
        say("| %s | %.1f | %.1f .. %.1f | %s |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, "" if bytes_moved is None else "%.2f" % (bytes_moved / t[0] / 1e12)))

    if args.scan_only:
        say("| what | ms (median of %d) | min .. max | |" % args.reps)
        say("|---|---|---|---|")
        for k, s in picked:
            a = automaton(k)
            row("am_contains_any_batch, %d needles (kept share %.1f %%)" % (k, 100 * s),
                timed(lambda: am.api.check(lib.am_contains_any_batch(a.device, case, b, flags.ctypes.data)), args.reps))
    else:
        sys.path.insert(0, HERE)
        from tests import select_reference as ref
        head = text[:min(total, 4 * 16384)].cpu().numpy()
        sample = [bytes(head[i * 2048:(i + 1) * 2048]) for i in range(32)]
        ss = am.api._Slices(sample)
        for k, _ in picked:
            for invert in (False, True):
                got = am.api._select(lambda out: lib.am_select_any(automaton(k).device, case, int(invert), ss.arr, ss.n, out))
                assert got.indices.tolist() == ref.keep(ref.pred_any(needles[:k], case), invert, sample)[0], ("select differs from the definition", k, invert)
        say("held to the definition first: the first 64 KiB as 32 haystacks, every measured subset, both senses: equal")
        say("")
        host_text = text[:total].cpu().numpy() if not args.lines else None
        src_offs = am.api.batch_offsets(b).astype(np.int64)
        if args.lines:
            host_text = np.zeros(total, np.uint8)
            am.api.check(lib.am_batch_read_text(b, 0, total, host_text.ctypes.data))
        lens = np.diff(src_offs)
        for k, s in picked:
            a = automaton(k)
            say("### %d needles: kept share %.2f %% of the haystacks" % (k, 100 * s))
            say("")
            say("| what | ms (median of %d) | min .. max | TB/s of kept text (read + written) |" % args.reps)
            say("|---|---|---|---|")
            state = {}

            def select_only():
                state["s"] = am.api._select(lambda out: lib.am_select_any_batch(a.device, case, 0, b, out))

            def gather_only():
                lib.am_batch_destroy(state["s"].batch(b))

            def whole():
                select_only()
                gather_only()

            t_whole = timed(whole, args.reps)
            t_sel = timed(select_only, args.reps)
            t_gather = timed(gather_only, args.reps)
            kept_bytes, kept = state["s"].total_bytes, state["s"].size
            kk = kernels(whole, ("select_plan", "select_emit", "select_gather"))
            t_scan = timed(lambda: am.api.check(lib.am_contains_any_batch(a.device, case, b, flags.ctypes.data)), args.reps)

            def host_route():
                am.api.check(lib.am_contains_any_batch(a.device, case, b, flags.ctypes.data))
                keep = flags[:n_src] != 0
                blob = host_text[np.repeat(keep, lens)]
                new_offs = np.zeros(int(keep.sum()) + 1, np.int64)
                np.cumsum(lens[keep], out=new_offs[1:])
                pad = torch.zeros((len(blob) + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
                pad[:len(blob)] = torch.from_numpy(blob).to(dev)
                d_offs = torch.from_numpy(new_offs).to(dev)
                torch.cuda.synchronize()
                nb = C.c_void_p()
                am.api.check(lib.am_batch_from_device(pad.data_ptr(), d_offs.data_ptr(), len(new_offs) - 1, len(blob), C.byref(nb)))
                lib.am_batch_destroy(nb)

            t_host = timed(host_route, min(args.reps, 2), warmup=0)
            src_copy = torch.empty(max(kept_bytes, 16), dtype=torch.uint8, device=dev)
            dst_copy = torch.empty_like(src_copy)

            def dtod():
                dst_copy.copy_(src_copy)
                torch.cuda.synchronize()

            t_copy = timed(dtod, args.reps)
            row("am_select_any_batch + am_batch_from_selection", t_whole)
            row("am_select_any_batch alone (scan, flags in HBM, compaction)", t_sel)
            row("am_batch_from_selection alone", t_gather, 2 * kept_bytes)
            row("am_contains_any_batch alone (scan, flags to the host)", t_scan)
            row("host route: am_contains_any_batch, numpy compaction, upload, am_batch_from_device", t_host)
            row("device-to-device copy of the kept bytes", t_copy, 2 * kept_bytes)
            say("")
            say("kept %d of %d haystacks, %d of %d bytes; kernels (HIP events): select_plan %.3f ms, select_emit %.3f ms, select_gather %.3f ms = %.2f TB/s of kept text (read + written)" % (
                kept, n_src, kept_bytes, total, kk["select_plan"], kk["select_emit"], kk["select_gather"],
                2 * kept_bytes / (kk["select_gather"] * 1e-3) / 1e12 if kk["select_gather"] > 0 else float("nan")))
            say("select / host route: %.1f ms / %.1f ms = %.1f x" % (t_whole[0] * 1e3, t_host[0] * 1e3, t_host[0] / t_whole[0]))
            say("")
            state.clear()
            del src_copy, dst_copy
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

"""Splitter on the device (am_split_batch, am_batch_from_fragments) next to the route it replaces, on three inputs:

  natural   --gib GiB of the natural-text workload in 1-MiB haystacks, split on "\\n".  synth's text has no line ends of its own: the blank after every full stop
            becomes one (on the device), so a line is a sentence of the workload;
  cfg3      the same size of cfg3's random code points, split on ",".  They hold no comma of their own: one ASCII byte in eight becomes one (on the device);
  chain     "aa" over --chain-mib MiB of 'a' in ONE haystack: every match overlaps the one before it, one chain through the whole text (pointer doubling).

For each: (a) am_split_batch, device-resident; (b) the route of the host mirror's splitBatch: am_run_batch + records to the host (am_matches_data: the wire-bound
part, reported by itself) + the host's fold (numpy, exact where separators cannot overlap; not run for `chain`), and (b') the host mirror's splitBatch itself from
host slices: am_run, the records to the host, stepAccum on one thread and a std::string per fragment; (c) am_count_batch on the same batch, the ceiling;
(d) am_split from host slices; (e) am_batch_from_fragments in GB/s of bytes moved (read + written) beside a plain device-to-device copy of the same bytes.
GiB/s are haystack bytes over the host clock around calls that end in a device synchronise (one warm-up, the median of --reps).  Kernel times: the library's HIP-event
brackets in a pass of their own, or `rocprofv3 --kernel-trace --stats -- python tests/measure/splitter.py --kernels-only`.  Run on the MI355X box:
    python tests/measure/splitter.py --gib 2 --out profiles/r08_splitter.md
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
    return float(np.median(ts))


def _prof(lib, key):
    ms, n = C.c_double(0), C.c_uint64(0)
    lib.am_profile_read(key.encode(), C.byref(ms), C.byref(n))
    return key, float(ms.value), int(n.value)


def measure(say, name, sep, text, n_bytes, hay_bytes, args, host_parts=True):
    import torch
    lib = am.api.libam()
    n_hay = n_bytes // hay_bytes
    offs = torch.arange(n_hay + 1, dtype=torch.int64, device=text.device) * hay_bytes
    sp = am.Splitter(sep)
    a = am.Automaton([sep])
    b = C.c_void_p()
    am.api.check(lib.am_batch_from_device(text.data_ptr(), offs.data_ptr(), n_hay, n_bytes, C.byref(b)))
    gib = n_bytes / float(1 << 30)
    sep_bytes = len(sep.encode())
    state = {}

    def run_a():
        if state.get("f"):
            lib.am_fragments_free(state["f"])
        state["f"] = sp.split_fragments(b)

    if args.kernels_only:
        for _ in range(3):
            run_a()
        nb = C.c_void_p()
        am.api.check(lib.am_batch_from_fragments(b, state["f"], C.byref(nb)))
        lib.am_batch_destroy(nb)
        lib.am_fragments_free(state["f"])
        lib.am_batch_destroy(b)
        return

    total = C.c_uint64(0)
    rows = [("(a) am_split_batch, device-resident", timed(run_a, args.reps))]
    rounds = int(lib.am_debug_split_rounds())
    n_frag = int(lib.am_fragments_size(state["f"]))
    rows.append(("(c) am_count_batch (ceiling)", timed(lambda: am.api.check(lib.am_count_batch(a.device, 0, b, None, C.byref(total))), args.reps)))

    parts = {"run": [], "copy": [], "fold": []}
    n_records = 0
    for rep in range(1 + min(args.reps, 3)):
        m = C.c_void_p()
        t0 = time.perf_counter()
        am.api.check(lib.am_run_batch(a.device, 0, b, C.byref(m)))
        t1 = time.perf_counter()
        n_records = int(lib.am_matches_size(m))
        p = lib.am_matches_data(m)
        assert p or not n_records
        t2 = time.perf_counter()
        t3 = t2
        if host_parts and n_records:
            # stepAccum where no two matches overlap: every record is kept; one thread, as splitBatch's fold is
            recs = np.frombuffer((C.c_char * (n_records * am.api.MATCH_DTYPE.itemsize)).from_address(p), dtype=am.api.MATCH_DTYPE)
            end = recs["end_pos"].astype(np.int64)
            first = np.flatnonzero(np.diff(recs["haystack"].astype(np.int64), prepend=-1))
            frag_start = np.concatenate(([0], end[:-1]))
            frag_start[first] = 0
            lens = end - sep_bytes - frag_start
            t3 = time.perf_counter()
            assert (lens >= 0).all() and len(lens) + n_hay == n_frag
        lib.am_matches_free(m)
        if rep:
            parts["run"].append(t1 - t0); parts["copy"].append(t2 - t1); parts["fold"].append(t3 - t2)
    tb = {k: float(np.median(v)) for k, v in parts.items()}
    rows.append(("(b) am_run_batch + records to the host%s" % (" + host fold (numpy, one thread)" if host_parts else ""), tb["run"] + tb["copy"] + tb["fold"]))
    rows.append(("    (b) am_run_batch alone (records stay in HBM)", tb["run"]))
    rows.append(("    (b) am_matches_data: %.2f GB of records over the wire" % (n_records * 16 / 1e9), tb["copy"]))
    rows.append(("    (b) wire-bound part: run + records over the wire", tb["run"] + tb["copy"]))
    if host_parts:
        rows.append(("    (b) host fold", tb["fold"]))

    if host_parts:
        host_text = text[:n_bytes].cpu().numpy()
        s = am.api._Slices([host_text[i * hay_bytes:(i + 1) * hay_bytes] for i in range(n_hay)])

        def run_d():
            f = C.c_void_p()
            am.api.check(lib.am_split(sp.device, 0, s.arr, s.n, C.byref(f)))
            assert int(lib.am_fragments_size(f)) == n_frag
            lib.am_fragments_free(f)

        rows.append(("(d) am_split from host slices", timed(run_d, min(args.reps, 3))))

        # (b) as the host mirror runs it from host slices: am_run, every record to the host, splitBatch's one-thread stepAccum with a std::string per fragment
        host = am.api.libhost()

        part = max(1, s.n // 8)                            # (an eighth of the haystacks, the time x 8: the fold builds a std::string per fragment)

        def run_mirror():
            blob, offs, nf = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
            per = np.zeros(part, np.uint32)
            am.api._hcheck(host.amh_splitter_split_batch(sp._h, 0, s.arr, part, C.byref(blob), C.byref(offs), C.byref(nf), per.ctypes.data))
            host.amh_free_blob(blob)
            host.amh_free_u64(offs)

        rows.append(("(b') host mirror splitBatch from host slices: am_run + records to the host + stepAccum + a std::string per fragment (on %d of the haystacks, "
                     "time x %d)" % (part, s.n // part), timed(run_mirror, 2) * (s.n // part)))
        del s, host_text

    say("### %s: %.2f GiB in %d haystacks of %d bytes, separator %r" % (name, gib, n_hay, hay_bytes, sep))
    say("")
    say("| what | ms | GiB/s of text |")
    say("|---|---|---|")
    for what, sec in rows:
        say("| %s | %.1f | %.1f |" % (what, sec * 1e3, gib / sec if sec > 0 else float("nan")))
    say("")
    say("%d records, %d fragments, %d rounds of pointer doubling" % (n_records, n_frag, rounds))

    # (e) the gather: bytes read + bytes written, beside a copy of the same bytes
    def run_e():
        nb = C.c_void_p()
        am.api.check(lib.am_batch_from_fragments(b, state["f"], C.byref(nb)))
        state["moved"] = int(lib.am_batch_total_bytes(nb))
        lib.am_batch_destroy(nb)

    te = timed(run_e, args.reps)
    moved = state["moved"]
    dst = torch.empty(max(moved, 1), dtype=torch.uint8, device=text.device)

    def run_copy():
        dst.copy_(text[:max(moved, 1)])
        torch.cuda.synchronize()

    tcopy = timed(run_copy, args.reps)
    say("")
    say("(e) am_batch_from_fragments: %d bytes into %d haystacks in %.1f ms = %.0f GB/s read + written (allocation and scan included); torch device-to-device copy of the same "
        "bytes: %.2f ms = %.0f GB/s" % (moved, n_frag, te * 1e3, 2 * moved / te / 1e9, tcopy * 1e3, 2 * moved / tcopy / 1e9))
    del dst

    am.api.check(lib.am_profile_enable(1))
    am.api.check(lib.am_profile_reset())
    run_a()
    run_e()
    keys = ("sf", "dfa", "dfa_place", "permute", "scan", "hidx", "split_start", "split_walk", "split_next", "split_double", "split_emit", "split_gather")
    say("")
    say("kernels of one am_split_batch + am_batch_from_fragments (HIP events): " + ", ".join("%s %.2f ms x %d" % r for r in (_prof(lib, k) for k in keys) if r[2]))
    say("")
    lib.am_profile_enable(0)
    lib.am_fragments_free(state["f"])
    lib.am_batch_destroy(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=2.0)
    ap.add_argument("--chain-mib", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="natural,cfg3,chain")
    ap.add_argument("--kernels-only", action="store_true", help="only (a) three times and one (e): the run to put under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    info = am.device_info()
    waves = am.api.resident_waves()
    say("## Splitter on the device")
    say("")
    say("%s, %d CUs, resident_waves_per_cu = %d" % (info["arch"], info["n_cu"], waves[0]))
    say("")
    n_cells = int(args.gib * (1 << 20))
    hay_bytes = 1 << 20
    if "natural" in args.only:
        w = synth.WORKLOADS["natural_100k_10GiB"]
        text, n_bytes = synth.haystacks_device(synth.needles_for("natural_100k_10GiB"), w["mixed"], 0, n_cells, dev, natural=True)
        ends = (text[:n_bytes - 1] == ord(".")) & (text[1:n_bytes] == ord(" "))
        text[1:n_bytes][ends] = ord("\n")
        del ends
        torch.cuda.synchronize()
        measure(say, "natural", "\n", text, n_bytes, hay_bytes, args)
        del text
    if "cfg3" in args.only:
        w = synth.WORKLOADS["cfg3_runLower_100k_10GiB"]
        text, n_bytes = synth.haystacks_device(synth.needles_for("cfg3_runLower_100k_10GiB")[:1000], w["mixed"], 0, n_cells, dev)
        # cfg3's random code points hold no comma: one ASCII byte in eight becomes one (seeded, on the device; multi-byte code points stay whole), about the
        # density of a CSV of short fields
        gen = torch.Generator(device=dev)
        gen.manual_seed(8)
        pick = (torch.randint(0, 8, (n_bytes,), dtype=torch.uint8, device=dev, generator=gen) == 0) & (text[:n_bytes] < 128)
        text[:n_bytes][pick] = ord(",")
        del pick
        torch.cuda.synchronize()
        measure(say, "cfg3 with commas", ",", text, n_bytes, hay_bytes, args)
        del text
    if "chain" in args.only:
        n_bytes = args.chain_mib << 20
        text = torch.full((n_bytes + 64,), ord("a"), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        measure(say, "chain", "aa", text, n_bytes, n_bytes, args, host_parts=False)
        del text
    if args.out and not args.kernels_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

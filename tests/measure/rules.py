"""Rule sets (am_rules_eval_batch) on a BASELINE workload reduced to --gib GiB, next to the two routes to the same answer that exist without them and to a plain copy
of the bytes the evaluation kernel moves:

  rules   rule sets of --rules rules drawn from the workload's dictionary (all_of of 2, any_of of 50, none_of of 1 a rule); n_slots is recorded;
  eval    the whole am_rules_eval_batch call by the host clock, and the kernel time of rules_eval from the library's HIP-event brackets (am_profile_*) in a pass of its
          own; the kernel's bytes are the slot rows read plus the `fired` words and the labels written;
  copy    a device-to-device copy (hipMemcpyDtoD through torch) of the same number of bytes;
  route 1 one am_select_all_batch / am_select_any_batch per clause group of a rule (all_of, any_of, none_of inverted): a SAMPLE of --sample rules is timed and the
          total for the rule set is EXTRAPOLATED from the sample's mean;
  route 2 am_count_matrix_batch over the union dictionary and the copy of its entries to the host (the Boolean algebra on the host is not timed), for rule sets of up
          to --matrix-max-rules rules;
  --contains-all-only  am_contains_all_batch alone over the first 3 needles of the dictionary -- with --root <tree> on another checkout, e.g. the parent commit built
          in a directory of its own, for the same-session comparison of containsAll before and after its slot rows were factored out.

--lines: the same text as a batch of its lines (Splitter("\\n").lines_batch, in HBM) instead of haystacks of --hay-kib KiB.
Before anything is timed the first 64 KiB are held to the definition (tests/rules_reference.py over the oracle).
Times are the host clock around calls that end in a device synchronise: a warm-up, then the median of --reps repetitions, with their minimum and maximum.  Run on the
MI355X box:
    python tests/measure/rules.py --workload natural_100k_10GiB --gib 2 --lines --out rules_lines.md
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
    ap.add_argument("--rules", default="10,100,1000")
    ap.add_argument("--sample", type=int, default=10, help="rules of a set that route 1 times")
    ap.add_argument("--matrix-max-rules", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--root", default=HERE, help="the checkout whose library is measured")
    ap.add_argument("--label", default="", help="what the heading calls the checkout, e.g. `parent`")
    ap.add_argument("--contains-all-only", action="store_true", help="am_contains_all_batch only (runs on a checkout without rule sets)")
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
    out_lines = []

    def say(s):
        print(s, flush=True)
        out_lines.append(s)

    def row(name, t, bytes_moved=None):
        say("| %s | %.1f | %.1f .. %.1f | %s |" % (name, t[0] * 1e3, t[1] * 1e3, t[2] * 1e3, "" if bytes_moved is None else "%.2f" % (bytes_moved / t[0] / 1e12)))

    info = am.device_info()
    say("## %s reduced to %.2f GiB as %s, case %d%s" % (args.workload, total / float(1 << 30), shape, case, " -- %s" % args.label if args.label else ""))
    say("")
    say("%s, %d CUs" % (info["arch"], info["n_cu"]))
    say("")
    flags = np.zeros(max(n_src, 1), np.uint8)
    words = [n for n in needles if n]
    if case:
        words = sorted(set(am.lower_utf8(n).decode("utf-8") for n in words))

    if args.contains_all_only:
        t = am.api.ValuesTable(am.Automaton(words[:3]))
        say("| what | ms (median of %d) | min .. max | |" % args.reps)
        say("|---|---|---|---|")
        row("am_contains_all_batch, 3 needles", timed(lambda: am.api.check(lib.am_contains_all_batch(t.handle, case, b, flags.ctypes.data)), args.reps))
        say("")
    else:
        sys.path.insert(0, HERE)
        from tests import rules_reference as ref
        head = text[:min(total, 4 * 16384)].cpu().numpy()
        sample = [bytes(head[i * 2048:(i + 1) * 2048]) for i in range(32)]

        def prof(key):
            ms, n = C.c_double(0), C.c_uint64(0)
            lib.am_profile_read(key.encode(), C.byref(ms), C.byref(n))
            return float(ms.value), int(n.value)

        for n_rules in [int(x) for x in args.rules.split(",")]:
            rng = random.Random(n_rules)
            specs = [(rng.sample(words, 2), rng.sample(words, 50), rng.sample(words, 1)) for _ in range(n_rules)]
            rs = am.RuleSet(case, [am.Rule(all_of=a, any_of=o, none_of=n) for a, o, n in specs])
            exp = ref.expect(rs.needles, rs.slots, rs.n_slots, case, ref.rules_of(rs.rule_off, rs.clause_off, rs.literals), sample)
            got = rs.eval(sample)
            assert np.array_equal(got.fired_words, exp[0]) and np.array_equal(got.labels, exp[2]) and np.array_equal(got.counts, exp[3]), "the rule set differs from the definition"
            say("### %d rules: %d needles, n_slots = %d (%d words a row)" % (n_rules, len(rs.needles), rs.n_slots, (rs.n_slots + 31) // 32))
            say("")
            say("held to the definition first: the first 64 KiB as 32 haystacks: equal")
            say("")
            say("| what | ms (median of %d) | min .. max | TB/s of the kernel's bytes |" % args.reps)
            say("|---|---|---|---|")
            state = {}

            def evaluate():
                state["hits"] = rs.eval_batch(b)

            t_eval = timed(evaluate, args.reps)
            am.api.check(lib.am_profile_enable(1))
            am.api.check(lib.am_profile_reset())
            try:
                evaluate()
                k_ms, k_n = prof("rules_eval")
            finally:
                lib.am_profile_enable(0)
            hits = state["hits"]
            fired_rules = int((hits.counts > 0).sum())
            labelled = int((hits.labels != am.api.RULE_NONE).sum())
            k_bytes = n_src * ((rs.n_slots + 31) // 32) * 4 + n_rules * hits.hay_words * 8 + n_src * 4
            state.clear()
            src_copy = torch.empty(max(k_bytes // 2, 16), dtype=torch.uint8, device=dev)
            dst_copy = torch.empty_like(src_copy)

            def dtod():
                dst_copy.copy_(src_copy)
                torch.cuda.synchronize()

            t_copy = timed(dtod, args.reps)
            del src_copy, dst_copy
            row("am_rules_eval_batch (scan, slot rows, evaluation)", t_eval)
            say("| rules_eval by its HIP events (%d launch%s) | %.3f | | %.2f |" % (k_n, "" if k_n == 1 else "es", k_ms, k_bytes / (k_ms * 1e-3) / 1e12 if k_ms > 0 else float("nan")))
            row("device-to-device copy of %d bytes read + written" % k_bytes, t_copy, k_bytes)
            # route 1: one select per clause group, a sample of the rules
            picked = specs[:min(args.sample, n_rules)]
            per_rule = []
            for a, o, n in picked:
                ta, ao, an = am.api.ValuesTable(am.Automaton(a)), am.Automaton(o), am.Automaton(n)

                def one_rule():
                    ta.select_all_batch(case, b)
                    am.api._select(lambda out: lib.am_select_any_batch(ao.device, case, 0, b, out))
                    am.api._select(lambda out: lib.am_select_any_batch(an.device, case, 1, b, out))

                per_rule.append(timed(one_rule, 1)[0])
            mean = float(np.mean(per_rule))
            say("| route 1: three selects a rule, %d rules timed | %.1f a rule | %.1f .. %.1f | |" % (len(picked), mean * 1e3, min(per_rule) * 1e3, max(per_rule) * 1e3))
            say("| route 1 for %d rules, EXTRAPOLATED from the sample's mean | %.1f | | |" % (n_rules, mean * n_rules * 1e3))
            # route 2: the term-document matrix of the union dictionary and its way to the host
            if n_rules <= args.matrix_max_rules:
                union = am.api.ValuesTable(am.Automaton(rs.needles))
                mstate = {}

                def matrix():
                    mstate["m"] = union.count_matrix_batch(case, b, raw=True)

                def wire():
                    mstate["e"] = am.api.matrix_to_numpy(mstate["m"])[1].shape[0]

                try:
                    t_mx = timed(matrix, 1, warmup=0)
                    t_wire = timed(wire, 1, warmup=0)
                    row("route 2: am_count_matrix_batch over the %d needles" % len(rs.needles), t_mx)
                    row("route 2: its %d entries (%d bytes) to the host" % (mstate["e"], mstate["e"] * 16), t_wire)
                    say("| route 2 in all (the Boolean algebra on the host not counted) | %.1f | | |" % ((t_mx[0] + t_wire[0]) * 1e3))
                    route2 = t_mx[0] + t_wire[0]
                except am.AmError as e:
                    say("| route 2: am_count_matrix_batch failed: %s | | | |" % e)
                    route2 = None
                finally:
                    if mstate.get("m"):
                        lib.am_needle_matrix_free(mstate["m"])
            else:
                route2 = None
                say("| route 2: not run for more than %d rules | | | |" % args.matrix_max_rules)
            say("")
            say("%d of %d rules fire somewhere, %d of %d haystacks carry a label; route 1 (extrapolated) / rule set = %.1f x%s" % (
                fired_rules, n_rules, labelled, n_src, mean * n_rules / t_eval[0], "" if route2 is None else "; route 2 / rule set = %.1f x" % (route2 / t_eval[0])))
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

"""The definition of am_near (include/am.h "proximity") in Python, brute force: for every anchor the minimum gap over ALL other spans of group_b in its haystack, a tie
to the lower index -- no previous / next shortcut, Python integers, no library call.  The spans come from tests/spans_reference.py (leftmost-longest over the oracle) or
tests/words_reference.py.  What the proximity tests expect -- never another path of the library."""
from oracle import oracle
from tests import spans_reference as sref

ORDERED = 1
ANYWHERE = 2 ** 64 - 1


def machine(needles, values=None):
    return oracle.Machine(list(needles), values)


def rows_of(needles, case, hays, values=None, n=None):
    """Per haystack the leftmost-longest (start, len, handle) rows."""
    return sref.spans(machine(needles, values), case, sref.LEFTMOST_LONGEST, needles, hays, n)


def near(rows, group_mask, queries, stats=None):
    """rows: per haystack a list of (start, len, handle); group_mask[handle]: bit g = in group g; queries: (group_a, group_b, max_gap, ordered).
    Returns (offsets [n_hay + 1], pairs [(a, b, gap, haystack, query)] with a / b global indices, fired [n_queries][n_hay] of bool, counts [n_queries]).
    stats (a dict, optional) counts what the anchors met: ties, partners on either side, anchors in both groups, lone anchors beside a neighbouring haystack's
    partner, gaps at and one beyond max_gap."""
    base, flat = [], []
    for r in rows:
        base.append(len(flat))
        flat += r

    def member(j, g):
        v = flat[j][2]
        return v < len(group_mask) and (group_mask[v] >> g) & 1 == 1

    n_hay, nq = len(rows), len(queries)
    offsets, pairs, fired, counts = [0], [], [[False] * n_hay for _ in range(nq)], [0] * nq
    groups = sorted(set(g for q in queries for g in q[:2]))
    for h, r in enumerate(rows):
        lo, hi = base[h], base[h] + len(r)
        members = {g: [j for j in range(lo, hi) if member(j, g)] for g in groups}      # every span of the group in this haystack
        found = []
        for q, (ga, gb, max_gap, ordered) in enumerate(queries):
            for i in members[ga]:
                best = None                                # (gap, index): the minimum over ALL other members in the haystack
                tied = False
                for j in members[gb]:
                    if j == i or (ordered and j < i):
                        continue
                    gap = flat[i][0] - (flat[j][0] + flat[j][1]) if j < i else flat[j][0] - (flat[i][0] + flat[i][1])
                    assert gap >= 0, "the rows overlap or descend"
                    if best is not None and gap == best[0]:
                        tied = True
                    if best is None or gap < best[0]:      # (ascending j: an equal gap later on does not replace the lower index)
                        best, tied = (gap, j), False
                if stats is not None:
                    _note(stats, best, tied, i, member(i, gb), ga != gb, max_gap, h, rows, group_mask, gb)
                if best is None or best[0] > max_gap:
                    continue
                found.append((i, best[1], best[0], h, q))
                fired[q][h] = True
                counts[q] += 1
        pairs += sorted(found, key=lambda p: (p[0], p[4]))   # rows ascend by (haystack, a, query)
        offsets.append(len(pairs))
    return offsets, pairs, fired, counts


def _note(stats, best, tied, i, anchor_in_b, two_groups, max_gap, h, rows, group_mask, gb):
    def bump(k):
        stats[k] = stats.get(k, 0) + 1
    if best is None:
        around = [rows[k] for k in (h - 1, h + 1) if 0 <= k < len(rows)]
        if any(v < len(group_mask) and (group_mask[v] >> gb) & 1 for r in around for _, _, v in r):
            bump("partner_only_next_door")
        return
    if best[0] == max_gap + 1:
        bump("gap_one_beyond")
    if best[0] > max_gap:
        return
    if tied:
        bump("tie")
    bump("partner_p" if best[1] < i else "partner_n")
    if anchor_in_b and two_groups:
        bump("anchor_in_both")
    if best[0] == max_gap:
        bump("gap_at_max")


def fired_words(fired, n_hay):
    """uint64 words per query as the C ABI lays them out (Python integers)."""
    hw = (n_hay + 63) // 64
    return [[sum(1 << (h % 64) for h in range(w * 64, min(n_hay, w * 64 + 64)) if row[h]) for w in range(hw)] for row in fired]


def readable(rows, pairs, n_queries):
    """Per haystack and query the pairs as (a_start, a_len, b_start, b_len, gap): what Automaton.near returns."""
    flat = [s for r in rows for s in r]
    out = [[[] for _ in range(n_queries)] for _ in rows]
    for a, b, gap, h, q in pairs:
        out[h][q].append((flat[a][0], flat[a][1], flat[b][0], flat[b][1], gap))
    return out

"""(CPU) What tests/test_gpu_postings_sort.py rests on (tests/postings_cases.py): the test library itself -- it cross-compiles for gfx950 and exports its C
interface and nothing else --, its limits and plans against am_postings_geometry and the splits the cases name, the numpy definitions against plain Python, the size
lists against the seams, the cost of a case, the patterns against what they are for, and the reporters against the defects they must see."""
import subprocess

import numpy as np

import alfred_margaret_amd as am
from tests import postings_cases as pc


def test_postcheck_builds_and_exports_its_interface():
    path = am.build.build_postcheck()
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    got = sorted(line.split()[-1] for line in out.splitlines() if " T " in line)
    assert got == ["ampc_bounds", "ampc_df", "ampc_gather", "ampc_guard_items", "ampc_hist", "ampc_keys", "ampc_limits", "ampc_offsets", "ampc_plan", "ampc_row_offsets", "ampc_scatter"]
    assert "build_postcheck" in am.build.build_all.__code__.co_names      # build_all() lists it


def test_limits_and_plans_are_the_librarys():
    lim = pc.limits()
    tile, wave, _, _ = am.api.postings_geometry(2)
    assert (lim.tile, lim.wave) == (tile, wave) and lim.tile == lim.wave * (lim.threads // pc.WAVE) and lim.wave % pc.WAVE == 0
    assert lim.max_spans == 0xFFFFFFFF and lim.row_threads % pc.WAVE == 0 and pc.guard() == 64
    for n_needles, split in pc.PLAN_SPLITS.items():
        pl = pc.plan(n_needles)
        assert (pl.passes, pl.bits[:pl.passes]) == (len(split), split), n_needles
        assert pl.shift[:pl.passes] == [sum(split[:k]) for k in range(len(split))] and pl.bits[pl.passes:] == [0] * (4 - pl.passes)
        if n_needles < 2 ** 32:                            # (the ABI's own report stops at 2^32 - 1 needles)
            assert am.api.postings_geometry(n_needles)[2:] == (len(split), split), n_needles
    assert am.api.postings_geometry(2 ** 32 - 1)[2:] == (4, [8, 8, 8, 8]) and pc.plan(2 ** 32).shift[3] == 24
    assert pc.plan(2 ** 40).bits == [8, 8, 8, 8]           # post_key_bits at its cap
    assert pc.plan(0).passes == 0 and pc.plan(1).passes == 0
    assert sorted(set(b for s in pc.PLAN_SPLITS.values() for b in s)) == list(range(1, 9))      # one pass of every digit width
    assert sorted(set(len(s) for s in pc.PLAN_SPLITS.values())) == [1, 2, 3, 4]


def test_size_lists_hold_every_seam_with_both_neighbours():
    lim = pc.limits()
    sizes = pc.sort_sizes(lim)
    for seam in pc.seams(lim):
        assert {seam - 1, seam, seam + 1} <= set(sizes), seam
    t, w, r = lim.tile, lim.wave, lim.row_threads
    assert min(sizes) == 0 and max(sizes) == 3 * t + w + 1 and 2 * t + 1 in sizes and len(set(sizes)) == len(sizes)
    assert pc.tiles(lim, max(sizes)) == 4 and [pc.tiles(lim, n) for n in (0, 1, t, t + 1)] == [0, 1, 1, 2]
    assert {r - 1, r, r + 1} <= set(pc.row_sizes(lim)) and set(sizes) <= set(pc.row_sizes(lim))
    assert {0, 1, r - 1, r, r + 1, 3 * r + 1} == set(pc.row_hay_counts(lim))
    assert {pc.WAVE, pc.WAVE + 1, r, r + 1} <= set(pc.lane_seams(lim))


def test_no_case_exceeds_its_budget():
    lim = pc.limits()
    n = max(pc.row_sizes(lim))
    assert pc.case_bytes(lim, n, cells=256 * pc.tiles(lim, n)) <= pc.MAX_CASE_BYTES
    assert max(pc.case_bytes(lim, len(keys), n_needles=nn) for _, keys, nn in pc.offsets_cases(lim)) <= pc.MAX_CASE_BYTES
    assert max(len(keys) for _, keys, _, _ in pc.df_cases(lim)) <= n
    assert max(len(h) for k in pc.row_hay_counts(lim) for _, h in pc.row_offsets_cases(lim, k)) * 24 <= pc.MAX_CASE_BYTES


# ---- the definitions against plain Python

def py_digit(pl, key, p):
    return (key >> pl.shift[p]) % (1 << pl.bits[p])


def test_the_sort_definitions_against_plain_python():
    lim = pc.limits()
    for n_needles in (8, 257, 65537, 2 ** 24 + 1, 2 ** 32):
        pl = pc.plan(n_needles)
        for n in (0, 1, 65, 300, lim.tile + 1):
            idx = pc.permutation(n)
            for p in range(pl.passes):
                for name, keys in pc.sort_patterns(lim, pl, p, n, n_needles):
                    ks, n_tiles = keys.tolist(), pc.tiles(lim, n)
                    assert pc.digit(pl, keys, p).tolist() == [py_digit(pl, k, p) for k in ks]
                    table = [0] * ((1 << pl.bits[p]) * n_tiles)
                    for i, k in enumerate(ks):
                        table[py_digit(pl, k, p) * n_tiles + i // lim.tile] += 1
                    counts = pc.hist_reference(lim, pl, p, keys)
                    assert counts.dtype == np.uint32 and counts.tolist() == table, (n_needles, n, p, name)
                    assert pc.bases(counts).tolist() == [sum(table[:c]) for c in range(len(table))] if len(table) <= 512 else True
                    order = sorted(range(n), key=lambda i: py_digit(pl, ks[i], p))      # (stable)
                    got_keys, got_idx = pc.scatter_reference(pl, p, keys, idx)
                    assert got_keys.tolist() == [ks[i] for i in order] and got_idx.tolist() == [int(idx[i]) for i in order], (n_needles, n, p, name)


def test_the_row_definitions_against_plain_python():
    lim = pc.limits()
    spans, idx = pc.random_spans(70), pc.permutation(70)
    data, source = pc.gather_reference(spans, idx)
    assert [data[k].tobytes() for k in range(70)] == [spans[int(i)].tobytes() for i in idx] and source.tolist() == [int(i) for i in idx] and source.dtype == np.uint64
    for name, keys, n_needles in pc.offsets_cases(lim):
        if len(keys) <= 300 and n_needles <= 300:
            ks = keys.tolist()
            assert pc.offsets_reference(keys, n_needles).tolist() == [sum(1 for k in ks if k < v) for v in range(n_needles + 1)], name
    assert pc.offsets_reference(np.zeros(0, np.uint32), 0).tolist() == [0] and pc.offsets_reference(np.asarray([0, 0, 2], np.uint32), 3).tolist() == [0, 2, 2, 3]
    for name, keys, hay, n_needles in pc.df_cases(lim):
        ks, hs = keys.tolist(), hay.tolist()
        assert ks == sorted(ks) and ks[-1] == n_needles - 1, name      # ascending, and key N - 1 present
        want = [0] * n_needles
        for k in range(len(ks)):
            if k == 0 or ks[k] != ks[k - 1] or hs[k] != hs[k - 1]:
                want[ks[k]] += 1
        got = pc.df_reference(keys, hay, n_needles)
        assert got.dtype == np.uint64 and got.tolist() == want, name
    for n_hay in pc.row_hay_counts(lim):
        for name, hay in pc.row_offsets_cases(lim, n_hay):
            hs = hay.tolist()
            assert hs == sorted(hs) and (not hs or hs[-1] < n_hay), (n_hay, name)
            want, k = [], 0
            for h in range(n_hay + 1):
                while k < len(hs) and hs[k] < h:
                    k += 1
                want.append(k)
            assert pc.row_offsets_reference(hay, n_hay).tolist() == want and want[-1] == len(hs), (n_hay, name)


# ---- the patterns are what they are for

def test_key_patterns():
    lim = pc.limits()
    t, w = lim.tile, lim.wave
    n = 2 * t + 1
    for n_needles in pc.PLAN_NEEDLES:
        pl = pc.plan(n_needles)
        for p in range(pl.passes):
            bits, d = pl.bits[p], 1 << pl.bits[p]
            full = pc.top_digit(pl, p, n_needles) == d - 1   # every digit value has a key below n_needles
            assert full or (p == pl.passes - 1 and n_needles & (n_needles - 1))
            got = dict(pc.sort_patterns(lim, pl, p, n, n_needles))
            assert len(got) == (10 if bits > 6 else 9)
            digits = {k: pc.digit(pl, v, p).astype(np.int64) for k, v in got.items()}
            for k, v in got.items():
                assert v.dtype == np.uint32 and len(v) == n and int(v.max()) < n_needles, (n_needles, p, k)
            if pl.passes > 1 or bits > 1:                    # equal digits, different keys: a swap shows in the keys too
                one = got["one value"]
                assert len(set(digits["one value"].tolist())) == 1 and (len(set(one.tolist())) > 1 or pc.key_bits(pl) == bits)
            if not full:
                continue
            assert set(digits["top bit alternating"].tolist()) == {0, d >> 1} and set(digits["lowest bit"].tolist()) == {d - 2, d - 1}
            every = digits["every value once per 2^bits"]
            for at in range(0, n - d, d):
                assert sorted(every[at:at + d].tolist()) == list(range(d))
            rounds = every[:n - n % 64].reshape(-1, 64)
            assert all(len(set(r.tolist())) == min(d, 64) for r in rounds)      # <= 6 bits: every value in one round; 7, 8: every lane another value
            lanes = np.arange(n) % 64
            assert ((digits["lane"] - lanes) % min(d, 64) == 0).all() and ((digits["63 - lane"] - (63 - lanes)) % min(d, 64) == 0).all()
            assert len(set(digits["lane"].tolist())) == d and len(set(digits["63 - lane"].tolist())) == d
            hot = np.bincount(digits["skewed"], minlength=d)
            assert hot[d - 1] > n // 16 or d <= 8
            runs = digits["seam runs"]
            change = np.flatnonzero(runs[1:] != runs[:-1]) + 1
            assert {63, 64, 65, w - 1, w, w + 1, t - 1, t, t + 1, 2 * t - 1, 2 * t} <= set(change.tolist()) or d == 1
            assert digits["a lone key in the last tile"][-1] == d - 1 and not digits["a lone key in the last tile"][:-1].any()
            if bits > 6:
                high = digits["values that differ above bit 5 only"]
                assert set((high % 64).tolist()) == {21} and len(set(high.tolist())) == d // 64
    assert "a lone key in the last tile" not in dict(pc.sort_patterns(lim, pc.plan(256), 0, t, 256))
    assert list(pc.sort_patterns(lim, pc.plan(256), 0, 0, 256))[0][1].shape == (0,)


def test_df_and_row_cases_sit_on_the_lane_seams():
    lim = pc.limits()
    r = lim.row_threads
    cases = {name: (keys, hay, nn) for name, keys, hay, nn in pc.df_cases(lim)}
    keys, hay, _ = cases["needle and haystack runs end on the same lane seams, N = 1009"]
    starts = set((np.flatnonzero(keys[1:] != keys[:-1]) + 1).tolist())
    assert starts == set(pc.lane_seams(lim)) == set((np.flatnonzero(hay[1:] != hay[:-1]) + 1).tolist())
    keys, hay, _ = cases["needle runs of 1, 64 and 65 rows, N = 1009"]
    assert {1, 64, 65} == set(np.diff(np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))).tolist())
    keys, hay, _ = cases["one needle run across a whole workgroup, one row per haystack, N = 1009"]
    assert len(set(keys[r - 3:2 * r + 5].tolist())) == 1 and keys[r - 4] != keys[r - 3] and keys[2 * r + 5] != keys[2 * r + 4] and len(set(hay.tolist())) == len(hay)
    keys, hay, nn = cases["one needle with one row per haystack over more than a workgroup, then another, N = 2"]
    assert int(pc.df_reference(keys, hay, nn)[0]) == r + 70 > r
    for n_hay in pc.row_hay_counts(lim)[3:]:
        got = dict(pc.row_offsets_cases(lim, n_hay))
        gaps = got["empty haystacks at the front, in the middle and at the end"]
        assert gaps[0] > 0 and gaps[-1] < n_hay - 1 and n_hay // 2 not in set(gaps.tolist()) and len(set(gaps.tolist())) > n_hay // 2
        present = set(got["four haystacks of five empty"].tolist())
        assert all(s in present and s - 1 in present for s in pc.lane_seams(lim) if s < n_hay) and len(present) < n_hay // 2


# ---- the reporters see what they are for

def scatter_model(lim, pl, p, keys, idx, drop_wave_prefix=False, tile_major=False):
    """What k_post_scatter computes, step by step in Python: dest = base[cell] + the keys of that digit in earlier wavefronts of the tile + in earlier rounds and lower
    lanes of its own.  With a defect switched on: the wavefronts before a lane's own not counted; the table indexed tile-major by both kernels."""
    n, n_tiles, digits = len(keys), pc.tiles(lim, len(keys)), 1 << pl.bits[p]
    cell = (lambda d, t: t * digits + d) if tile_major else (lambda d, t: d * n_tiles + t)
    ds = pc.digit(pl, keys, p).tolist()
    counts = np.zeros(digits * n_tiles, np.uint32)
    for i, d in enumerate(ds):
        counts[cell(d, i // lim.tile)] += 1
    base = pc.bases(counts)
    keys_out, idx_out = pc.fresh(n, np.uint32), pc.fresh(n, np.uint32)
    for t in range(n_tiles):
        before = [0] * digits                              # keys of the digit in earlier wavefronts of this tile
        for w0 in range(t * lim.tile, min((t + 1) * lim.tile, n), lim.wave):
            mine = [0] * digits
            for i in range(w0, min(w0 + lim.wave, n)):
                d = ds[i]
                dest = int(base[cell(d, t)]) + (0 if drop_wave_prefix else before[d]) + mine[d]
                mine[d] += 1
                if dest < n:
                    keys_out[dest], idx_out[dest] = keys[i], idx[i]
            before = [a + b for a, b in zip(before, mine)]
    return counts, keys_out, idx_out


def test_reporters_see_the_defects_they_are_for():
    lim = pc.limits()
    n = 2 * lim.tile + 1
    for n_needles, p in ((256, 0), (65537, 1), (2 ** 24 + 1, 0)):
        pl = pc.plan(n_needles)
        idx = pc.permutation(n)
        for name, keys in pc.sort_patterns(lim, pl, p, n, n_needles):
            good_counts = np.concatenate([pc.hist_reference(lim, pl, p, keys), pc.fresh(0, np.uint32)])
            assert pc.hist_mismatch(lim, pl, p, keys, good_counts, name) is None
            counts, keys_out, idx_out = scatter_model(lim, pl, p, keys, idx)
            assert counts.tolist() == good_counts[:len(counts)].tolist()
            assert pc.scatter_mismatch(pl, p, keys, idx, keys_out, idx_out, name) is None, name      # the model of the kernel IS the stable sort
            # a swap of two neighbours with the same digit value
            ds = pc.digit(pl, keys_out[:n], p)
            at = int(np.flatnonzero(ds[1:] == ds[:-1])[0])
            bad_keys, bad_idx = keys_out.copy(), idx_out.copy()
            bad_keys[[at, at + 1]], bad_idx[[at, at + 1]] = keys_out[[at + 1, at]], idx_out[[at + 1, at]]
            assert "idx_out[%d]" % at in pc.scatter_mismatch(pl, p, keys, idx, keys_out, bad_idx, name)
            if bad_keys[at] != keys_out[at]:
                assert "keys_out[%d]" % at in pc.scatter_mismatch(pl, p, keys, idx, bad_keys, idx_out, name)
            # the second wavefront's keys of a digit written over the first's
            _, lost_keys, lost_idx = scatter_model(lim, pl, p, keys, idx, drop_wave_prefix=True)
            where = set(zip((np.arange(n) // lim.tile).tolist(), pc.digit(pl, keys, p).tolist(), (np.arange(n) // lim.wave).tolist()))
            shared = len(where) > len({(t, d) for t, d, _ in where})      # some digit value occurs in two wavefronts of one tile
            assert (pc.scatter_mismatch(pl, p, keys, idx, lost_keys, lost_idx, name) is not None) == shared, name
            assert shared or name == "seam runs", name
            # a tile-major table, consistently in both kernels: the table is wrong, and so is the order its sum gives
            major_counts, major_keys, major_idx = scatter_model(lim, pl, p, keys, idx, tile_major=True)
            major_counts = np.concatenate([major_counts, pc.fresh(0, np.uint32)])
            if len(set(pc.digit(pl, keys, p).tolist())) > 1:
                assert "counts[" in pc.hist_mismatch(lim, pl, p, keys, major_counts, name), name
                ascending = bool((np.diff(pc.digit(pl, keys, p).astype(np.int64)) >= 0).all())      # (in order as it is: every table leaves it so)
                assert (pc.scatter_mismatch(pl, p, keys, idx, major_keys, major_idx, name) is None) == ascending, name
                assert not ascending or name == "a lone key in the last tile"
    # the guards, and every other reporter on one wrong element
    keys = np.sort(pc.permutation(100) % 7).astype(np.uint32)
    hay = np.arange(100, dtype=np.uint32) // 3
    spans, idx = pc.df_rows(keys, hay), pc.permutation(100)
    good = {
        "offsets": (np.concatenate([pc.offsets_reference(keys, 7), pc.fresh(0, np.uint64)]), lambda o: pc.offsets_mismatch(keys, 7, o, "x")),
        "doc_freq": (np.concatenate([pc.df_reference(keys, hay, 7), pc.fresh(0, np.uint64)]), lambda o: pc.df_mismatch(keys, hay, 7, o, "x")),
        "out_off": (np.concatenate([pc.row_offsets_reference(hay, 40), pc.fresh(0, np.uint64)]), lambda o: pc.row_offsets_mismatch(hay, 40, o, "x")),
        "source": (np.concatenate([idx.astype(np.uint64), pc.fresh(0, np.uint64)]),
                   lambda o: pc.gather_mismatch(spans, idx, np.concatenate([spans[idx], pc.fresh(0, pc.SPAN)]), o, "x")),
        "idx": (np.concatenate([np.arange(100, dtype=np.uint32), pc.fresh(0, np.uint32)]),
                lambda o: pc.keys_mismatch(spans, np.concatenate([keys, pc.fresh(0, np.uint32)]), o, "x")),
    }
    for word, (out, report) in good.items():
        assert report(out) is None, word
        n_own = len(out) - pc.guard()
        for at, seen in ((0, word + "[0]"), (n_own - 1, "%s[%d]" % (word, n_own - 1)), (n_own, "guard"), (len(out) - 1, "guard")):
            bad = out.copy()
            bad[at] += 1
            assert seen in report(bad), (word, at)
        assert "elements" in report(out[:-1])
    data = np.concatenate([spans[idx], pc.fresh(0, pc.SPAN)])
    source = good["source"][0]
    assert pc.gather_mismatch(spans, idx, data, source, "x") is None
    for field in ("start", "len", "haystack", "needle"):     # all 24 bytes of a row
        bad = data.copy()
        bad[field][17] ^= 1
        assert "data[17]" in pc.gather_mismatch(spans, idx, bad, source, "x")
    bad = data.copy()
    bad["len"][100] ^= 1
    assert "guard" in pc.gather_mismatch(spans, idx, bad, source, "x")
    assert pc.untouched(pc.fresh(5, pc.SPAN)) and not pc.untouched(bad[100:])

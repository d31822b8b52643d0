"""The inputs and the plain reference of tests/test_gpu_dense_units.py (automata with the empty needle, csrc/am_dense.hip k_dense), checked on the CPU: the
reference of tests/helpers.py against the oracle and the naive oracle, the constructed batches for what they claim to hold, the unit geometry the GPU tests
sit on (am_debug_sf_unit_chunks), and a numpy model of the write pass's rank arithmetic that three wrong kernels do not survive."""
import random

import numpy as np
import pytest

import alfred_margaret_amd as am
from oracle import naive, oracle
from tests.helpers import DENSE_CHUNK, DENSE_ONLY_SETS, DENSE_SETS, dense_placements, dense_reference, dense_text, ragged_cuts

MIB = 1 << 20
# the batch sizes of the GPU tests and the unit_chunks they give on 256 compute units (16 wavefronts each)
GPU_SHAPES = ((3 * MIB + 77, 1), (4 * MIB + 4096 + 19, 2), (32 * MIB, 8), (36 * MIB - 13, 9), (256 * MIB, 64), (256 * MIB + 64 * 1024 + 5, 33))


@pytest.fixture(scope="module")
def batches():
    """{set name: (text, offsets)}: 1 MiB of dense_text cut by ragged_cuts, one-chunk units."""
    out = {}
    for name, (_, _, alphabet) in DENSE_SETS.items():
        rng = random.Random(11)
        text = dense_text(rng, MIB, alphabet)
        out[name] = (text, ragged_cuts(text, rng, DENSE_CHUNK, big=300 << 10))
    return out


def reference_of_oracle(case, needles, text, offs):
    """(haystack, end_pos, n_values) of the oracle's fold: consecutive values at one position collapse into one entry."""
    m = oracle.Machine(needles)
    t = np.frombuffer(text, dtype=np.uint8)
    hay, end, cnt = [], [], []
    for i in range(len(offs) - 1):
        pos, _ = m.run_list(case, t, int(offs[i]), int(offs[i + 1] - offs[i]))
        u, c = np.unique(pos.astype(np.int64), return_counts=True)
        assert np.array_equal(np.repeat(u, c), pos.astype(np.int64))          # fold order is position order
        hay.append(np.full(len(u), i, dtype=np.int64)); end.append(u); cnt.append(c)
    return np.concatenate(hay), np.concatenate(end), np.concatenate(cnt)


SETS = [(name, case, needles) for name, (case, needles, _) in DENSE_SETS.items()] + \
       [(text_of, case, needles) for (case, needles), text_of in zip(DENSE_ONLY_SETS.values(), ("sensitive", "sensitive"))]      # its text holds É and é


@pytest.mark.parametrize("text_of,case,needles", SETS, ids=[n for n in DENSE_SETS] + [n for n in DENSE_ONLY_SETS])
def test_dense_reference_equals_the_oracle_on_every_haystack(batches, text_of, case, needles):
    text, offs = batches[text_of]
    for c in ((case,) if needles in [v[1] for v in DENSE_ONLY_SETS.values()] else (0, 1)):       # the main sets under both case modes
        got = dense_reference(c, needles, text, offs)
        exp = reference_of_oracle(c, needles, text, offs)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp)), (text_of, c, len(got[0]), len(exp[0]))
        if len(needles) > 2 and c == case:
            assert len(got[0]) > len(text) // 8 and (got[2] > 1).sum() > len(text) // 200      # dense, and a few percent complete a needle


def test_only_the_dense_part_means_no_record():
    """{""} alone, and an upper-case needle under IgnoreCase: no goto ever succeeds, the reference folds nothing."""
    text = dense_text(random.Random(5), 4096, DENSE_SETS["sensitive"][2])
    for case, needles in DENSE_ONLY_SETS.values():
        assert len(dense_reference(case, needles, text, [0, len(text)])[0]) == 0


@pytest.mark.parametrize("name", list(DENSE_SETS))
def test_dense_reference_equals_the_naive_oracle_on_a_slice(batches, name):
    """oracle/naive.py knows no empty needle: its matches are the values beyond the root's at every position."""
    case, needles, _ = DENSE_SETS[name]
    text, _ = batches[name]
    cut = 64 << 10
    while (text[cut] & 0xC0) == 0x80:
        cut -= 1
    _, end, n_values = dense_reference(case, needles, text[:cut], [0, cut])
    exp = np.asarray([e for e, _ in naive.all_matches(needles[1:], text[:cut].decode("utf-8"), bool(case))], dtype=np.int64)
    assert len(exp) > 500 and np.array_equal(np.repeat(end, n_values - 1), exp)


@pytest.mark.parametrize("name", list(DENSE_SETS))
def test_the_batches_hold_what_they_claim(batches, name):
    case, needles, _ = DENSE_SETS[name]
    text, offs = batches[name]
    t = np.frombuffer(text, dtype=np.uint8)
    assert offs[0] == 0 and offs[-1] == len(text) and (np.diff(offs) >= 0).all()
    assert ((t[offs[:-1][offs[:-1] < len(t)]] & 0xC0) != 0x80).all()          # cuts on code-point boundaries only
    text.decode("utf-8")
    lens = set(np.diff(offs).tolist())
    assert {0, 1, 2, 3, 5} <= lens and max(lens) >= 250 << 10 and any(1021 <= x <= 1025 for x in lens) and any(65533 <= x <= 65537 for x in lens)
    got = dense_placements(case, needles, text, offs, DENSE_CHUNK)
    for what in ("first ends a word", "first ends on the first byte of a word", "first ends a unit", "first ends a haystack and a word", "words with three haystacks",
                 "empty haystacks inside a word"):
        assert got[what] >= 1, (what, got)
    assert 0.30 <= got["first share"] <= 0.70, got
    n_multi = sum(1 for c, _ in DENSE_SETS[name][2] if len(c.encode("utf-8")) > 1)
    assert {len(c.encode("utf-8")) for c, _ in DENSE_SETS[name][2]} >= ({1, 2, 3, 4} if not case else {1, 2, 3}) and n_multi >= 4


def test_unit_geometry_of_the_gpu_shapes():
    """am_debug_sf_unit_chunks is pure with n_cu > 0 (no device): the sizes of tests/test_gpu_dense_units.py reach 1, 2, 8, 9, 64 and 33 chunks per unit on 256
    compute units, and no batch up to 4 GiB gets a unit beyond k_dense's bitmap (launch_dense: unit_chunks * 32 words <= 2048)."""
    assert "am_debug_sf_unit_chunks" in am.api.DEBUG_ABI
    assert [am.api.sf_unit_chunks(total, 256) for total, _ in GPU_SHAPES] == [uc for _, uc in GPU_SHAPES]
    assert am.api.sf_unit_chunks(3 * MIB + 77, 256) == 1 and (3 * MIB + 77 + 1023) // 1024 >= 3000
    waves = 256 * 16
    sizes = set()
    for k in range(0, 1025):                                                  # every multiple of 4 MiB (one chunk per wavefront more), and its neighbours
        sizes.update(max(1, k * waves * 1024 + d) for d in (-1025, -1, 0, 1, 1024, 1025))
    sizes.update(1 << s for s in range(0, 33))
    for n_cu in (256, 304, 1, 64):
        worst = max(am.api.sf_unit_chunks(min(total, 4 << 30), n_cu) for total in sizes)
        assert 1 <= worst and worst * (DENSE_CHUNK // 32) <= 2048, (n_cu, worst)
    assert am.api.sf_unit_chunks(4 << 30, 256) == 64


# ---- the write pass of k_dense as numpy (am_dense.hip: `per`, un_pre / sp_pre, the rank of a position inside its word), and three wrong kernels

def write_pass(un_bits, sp_bits, sparse, per_of=lambda n_words: (n_words + 255) // 256, below_of=lambda j: (1 << j) - 1):
    """The slots k_dense<.., true> writes for ONE unit: un_bits / sp_bits = the unit's bitmap words, sparse = its k_sf records (any labels).  Returns the output as a
    list: a sparse record's label, or ("dense", position)."""
    n_words = len(un_bits)
    per = per_of(n_words)
    popc = lambda x: bin(int(x)).count("1")
    cu, cs = [0] * 256, [0] * 256
    for t in range(256):
        for w in range(min(t * per, n_words), min((t + 1) * per, n_words)):
            cu[t] += popc(un_bits[w]); cs[t] += popc(sp_bits[w])
    un_pre, sp_pre = [None] * n_words, [None] * n_words
    for t in range(256):
        run_un, run_sp = sum(cu[:t]), sum(cs[:t])
        for w in range(min(t * per, n_words), min((t + 1) * per, n_words)):
            un_pre[w], sp_pre[w] = run_un, run_sp
            run_un += popc(un_bits[w]); run_sp += popc(sp_bits[w])
    out = {}
    for p in range(32 * n_words):
        w, j = p >> 5, p & 31
        if not (int(un_bits[w]) >> j) & 1 or un_pre[w] is None:
            continue
        at = un_pre[w] + popc(int(un_bits[w]) & below_of(j))
        out[at] = sparse[sp_pre[w] + popc(int(sp_bits[w]) & below_of(j))] if (int(sp_bits[w]) >> j) & 1 else ("dense", p)
    return [out.get(i) for i in range(sum(popc(x) for x in un_bits))]


@pytest.mark.parametrize("n_words", (32, 256, 288, 2048))
def test_rank_arithmetic_of_the_write_pass_and_two_wrong_ones(n_words):
    """The model places every position of a unit in position order; with `per = n_words / 256` (words beyond 256 * per are never summed) or `below = 1 << j`
    (a position ranked by its own bit alone) it does not, at the word counts the GPU shapes reach: 288 is the first with per = 2."""
    rng = np.random.default_rng(n_words)
    un = rng.integers(0, 1 << 32, n_words, dtype=np.uint64)
    sp = un & rng.integers(0, 1 << 32, n_words, dtype=np.uint64) & rng.integers(0, 1 << 32, n_words, dtype=np.uint64)
    pos = [p for p in range(32 * n_words) if (int(un[p >> 5]) >> (p & 31)) & 1]
    is_sp = [(int(sp[p >> 5]) >> (p & 31)) & 1 for p in pos]
    sparse = [("sparse", p) for p, s in zip(pos, is_sp) if s]
    exp = [("sparse", p) if s else ("dense", p) for p, s in zip(pos, is_sp)]
    assert write_pass(un, sp, sparse) == exp
    if n_words % 256:
        assert write_pass(un, sp, sparse, per_of=lambda n: n // 256) != exp
    assert write_pass(un, sp, sparse + [None] * 64, below_of=lambda j: 1 << j) != exp

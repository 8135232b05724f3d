"""CPU proof of tests/_update.py, the yardstick of tests/test_gpu_update.py: on every named case the definition (the blend on
unpacked bits), the decode of the reference streams and the kernel's restated arithmetic are one bitmap; the
wah_update_max_words bound holds on the named cases, foreign re-encodings among them, and on 200 random draws; every named case
reaches what its name says; and each of four wrong models of the arithmetic changes an answer on a named case."""
import numpy as np
import pytest

from tests import _foreign, _select, _update as up

SEG_WORDS, SEG_BITS = up.SEG_WORDS, up.SEG_BITS
CASES = up.named_cases()
FOREIGN = up.foreign_cases()
ALL = CASES + FOREIGN


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_definition_reference_and_arithmetic_agree(oracle, case):
    stream, index = up.reference(oracle, case)
    segments = _select.segments_of(case.n_words)
    assert index.size == case.n_columns * segments + 1 and index[-1] == stream.size
    sel = case.selection()
    for c in range(case.n_columns):
        want = up.model(case, c)
        own = stream[index[c * segments]: index[(c + 1) * segments]]
        assert np.array_equal(np.asarray(oracle.decompress(own), np.uint32)[: case.n_words], want), (case.name, c)
        assert np.array_equal(up.arithmetic(case, c), up.model_groups(case, c)), (case.name, c)
        bits = up.bits_of(want)
        assert np.array_equal(bits[sel == 1], up.bits_of(case.words("then", c))[sel == 1])
        assert np.array_equal(bits[sel == 0], up.bits_of(case.words("else", c))[sel == 0])


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_the_streams_are_what_the_case_says(oracle, case):
    """A foreign way decodes to the same bitmap (but for the set pad bits); a constant has no stream."""
    streams = [(case.mask, case.mask_stream(oracle), case.mask_way)]
    for side in ("else", "then"):
        for c in range(case.n_columns):
            st = case.stream(oracle, side, c)
            assert (st is None) == (case.constant(side, c) is not None)
            if st is not None:
                streams.append((case.sides[side][c], st, case.ways[side][c]))
    for words, st, way in streams:
        back = np.asarray(oracle.decompress(st), np.uint32)[: case.n_words]
        if way in _foreign.PAD_WAYS:
            assert np.array_equal(back[:-1], words[:-1])
            assert int(st[-1]) & up.FILL0 or int(st[-1]) & (up.M31 ^ (up.M31 >> _foreign.pad_bits(case.n_words))), "set pad bits"
        else:
            assert np.array_equal(back, words), (case.name, way)
        assert _foreign.segment_ranges(st)[1] == _select.groups_of(case.n_words)


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_max_words_bounds_the_named_cases(oracle, case):
    stream, _ = up.reference(oracle, case)
    bound = up.max_words(case.n_words, case.n_columns, *up.read_words(oracle, case))
    assert stream.size <= bound, (case.name, stream.size, bound)


def _runs(rng, n_bits, density, run):
    """Bits in runs of mean length `run`, a share `density` of them set."""
    n_runs = max(int(2.5 * n_bits / run), 8)
    lengths = rng.geometric(1.0 / run, n_runs)
    values = (rng.random(n_runs) < density).astype(np.uint8)
    bits = np.repeat(values, lengths)
    while bits.size < n_bits:
        bits = np.concatenate([bits, bits])
    return bits[:n_bits]


@pytest.mark.parametrize("seed", range(8))
def test_max_words_bounds_random_draws(oracle, seed):
    """25 draws per seed, 200 in all, of (densities, run lengths, constants, row limit) over 1 .. 3 segments, ragged ones among
    them: the words of the output against the bound for the words that are read."""
    rng = np.random.default_rng([seed, 78])
    for draw in range(25):
        n = int(rng.integers(1, 4)) * SEG_WORDS + int(rng.integers(0, 2)) * int(rng.integers(1, 40))
        entries = []
        for _ in range(3):
            d, r = float(rng.choice([0.001, 0.03, 0.5, 0.97, 0.999])), float(rng.choice([1, 3, 31, 40, 62, 500, 5000, 40000]))
            entries.append(up.words_of(_runs(rng, 32 * n, d, r)))
        mask, else_, then = entries
        kind = int(rng.integers(0, 6))
        if kind == 0:
            then = int(rng.integers(0, 2))
        elif kind == 1:
            else_ = int(rng.integers(0, 2))
        elif kind == 2:
            else_, then = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        n_rows = 32 * n - int(rng.integers(0, 2)) * int(rng.integers(0, 32 * n + 1))
        case = up.Case(f"draw {seed}.{draw}", n, n_rows, mask, [else_], [then])
        out = np.ascontiguousarray(oracle.compress(up.model(case, 0)), dtype=np.uint32)
        bound = up.max_words(n, 1, *up.read_words(oracle, case))
        assert out.size <= bound, (case.name, out.size, bound, n, n_rows, kind)
        assert np.array_equal(up.arithmetic(case, 0), up.model_groups(case, 0)), case.name


def test_the_bound_needs_its_three_words():
    """Constants on both sides under a mask of one fill: the words are those the row limit and the pad bits make -- ones up to
    the row limit's group, that group, zeros behind it; with constant ones on the else side the last group is set apart."""
    n = SEG_WORDS + 1
    ones = np.full(n, up.ONES, np.uint32)
    clip = up.Case("clip", n, 31 * 500 + 7, ones, [0], [1])
    assert np.count_nonzero(np.diff(up.model_groups(clip, 0).astype(np.int64))) == 2  # three runs in segment 0, one word in segment 1
    pad = up.Case("pad", n, 0, np.zeros(n, np.uint32), [1], [0])
    groups = up.model_groups(pad, 0)
    assert (groups[:-1] == up.M31).all() and groups[-1] == up.M31 >> _foreign.pad_bits(n)


def test_named_cases_reach_what_their_names_say(oracle):
    assert not up.mask_of_zeros().selection().any() and up.selecting_segments(up.mask_of_zeros()) == []
    ones = up.mask_of_ones()
    assert ones.selection().all() and _select.pad_bits(ones.n_words)
    fills = up.fill_mask_segments()
    st = fills.mask_stream(oracle)
    assert st.size == 3 and all(int(w) & up.FILL0 for w in st) and up.selecting_segments(fills) == [1]
    seams = up.seam_rows()
    rows = np.flatnonzero(seams.selection())
    assert {31 * 63 + 30, 31 * 64, SEG_BITS - 1, SEG_BITS, 32 * seams.n_words - 1} <= set(rows.tolist())
    assert (31 * 63 + 30) // 31 % 64 == 63 and (31 * 64) // 31 % 64 == 0
    assert up.selecting_segments(up.sparse_mask()) == [0, 2]
    same = up.same_operand()
    for c in range(same.n_columns):
        assert np.array_equal(up.model(same, c), same.words("else", c))
    both = up.constants("both")
    assert {(both.constant("else", c), both.constant("then", c)) for c in range(4)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for n_rows in up.ROW_LIMITS:
        assert up.row_limit(n_rows).n_rows == n_rows
    assert up.row_limit(None).n_rows == 32 * up.row_limit(None).n_words
    for way in _foreign.PAD_WAYS:
        assert _select.pad_bits(up.set_pad_bits(way).n_words)
    assert up.full_grid_columns() > up.GRID_CAP * up.SEG_WAVES
    assert len(FOREIGN) == 3 * (len(_foreign.WAYS) - 1)


def test_the_grid_cap_is_the_launcher_s():
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-wah_amd", "csrc", "wah_update.hip")
    with open(path) as f:
        body = f.read().split("hipError_t launch_update_segments", 1)[1]
    a, b = re.search(r"most = (\d+)u \* (\d+)u;", body).groups()
    assert int(a) * int(b) == up.GRID_CAP


WRONG_ON = {
    "rows at or behind n_rows updated": lambda: up.row_limit(31 * 700 + 7),
    "pad bits carried": lambda: up.set_pad_bits(),
    "constant ones written outside the mask": lambda: up.constants("then"),
    "then and else swapped where the mask segment is a fill": lambda: up.fill_mask_segments(),
}


@pytest.mark.parametrize("wrong", up.WRONG_MODELS)
def test_a_wrong_model_changes_an_answer(wrong):
    case = WRONG_ON[wrong]()
    changed = False
    for c in range(case.n_columns):
        right = up.arithmetic(case, c)
        assert np.array_equal(right, up.model_groups(case, c))
        changed |= not np.array_equal(up.arithmetic(case, c, wrong), right)
    assert changed, wrong


def test_a_wrong_model_is_caught_by_a_case_the_gpu_runs():
    """Every wrong model differs from the right one on at least one of the named cases."""
    for wrong in up.WRONG_MODELS:
        assert any(not np.array_equal(up.arithmetic(case, c, wrong), up.arithmetic(case, c)) for case in CASES for c in range(case.n_columns)), wrong


def test_sizes_by_hand():
    assert up.scratch_bytes(1, 1) == 1024 + 256 + 256
    assert up.scratch_bytes(992 * 4, 3) == 1536
    # 64 x 1024 + 1 index entries: 17 level-1 entries
    assert up.scratch_bytes(1024 * SEG_WORDS, 64) == 1024 + 256 + 256
    # one segment of 1024 groups, 3 columns: all literals 3072; by words 100 + 3 * (10 + 3) = 139
    assert up.max_words(SEG_WORDS, 3, 10, 100) == 139
    assert up.max_words(SEG_WORDS, 3, 1000, 100) == 3072
    assert up.max_words(1, 1, 1 << 63, 1 << 63) == 2

"""CPU proof of tests/_compact.py, the yardstick of tests/test_gpu_compact.py: on every named case the definition (rows picked
out of unpacked bits), the decode of the reference streams and the kernel's restated arithmetic are one bitmap; the
wah_compact_max_words bound holds on the named cases and on a few hundred random draws; every named case reaches what its name
says; and each of four wrong models of the arithmetic changes an answer on a named case."""
import numpy as np
import pytest

from tests import _compact as cp, _foreign, _select

SEG_WORDS, SEG_BITS = cp.SEG_WORDS, cp.SEG_BITS
CASES = cp.named_cases()
FOREIGN = [cp.foreign(way) for way in _foreign.WAYS[1:]]


@pytest.mark.parametrize("case", CASES + FOREIGN, ids=[c.name for c in CASES + FOREIGN])
def test_definition_reference_and_arithmetic_agree(oracle, case):
    stream, index, total = cp.reference(oracle, case)
    assert total == int(cp.ranks(case)[-1]) == case.total_rows
    segments = _select.segments_of(case.n_words_out)
    assert index.size == case.n_columns * segments + 1 and index[-1] == stream.size
    for c in range(case.n_columns):
        want = cp.model(case, c)
        own = stream[index[c * segments]: index[(c + 1) * segments]]
        assert np.array_equal(np.asarray(oracle.decompress(own), np.uint32)[: case.n_words_out], want), (case.name, c)
        assert np.array_equal(cp.arithmetic(case, c), want), (case.name, c)
        assert not cp.bits_of(want)[total:].any()


@pytest.mark.parametrize("case", CASES + FOREIGN, ids=[c.name for c in CASES + FOREIGN])
def test_the_streams_are_what_the_case_says(oracle, case):
    """A foreign way decodes to the same bitmap (but for the set pad bits) and differs from compress() where it should."""
    for words, st, way in [(case.mask, case.mask_stream(oracle), case.mask_way)] + [
            (case.columns[c], case.column_stream(oracle, c), case.column_ways[c]) for c in range(case.n_columns)]:
        back = np.asarray(oracle.decompress(st), np.uint32)[: case.n_words]
        if way in _foreign.PAD_WAYS:
            assert np.array_equal(back[:-1], words[:-1])
            groups = _foreign.unpack(back)  # (what the stream holds in the pad bits is visible only in its last word)
            assert groups.size == _select.groups_of(case.n_words)
        else:
            assert np.array_equal(back, words), (case.name, way)
        assert _foreign.segment_ranges(st)[1] == _select.groups_of(case.n_words)


@pytest.mark.parametrize("case", CASES + FOREIGN, ids=[c.name for c in CASES + FOREIGN])
def test_max_words_bounds_the_named_cases(oracle, case):
    stream, _, _ = cp.reference(oracle, case)
    assert stream.size <= cp.max_words(case.n_words_out, case.n_columns, cp.read_source_words(oracle, case)), case.name


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
    """40 draws per seed of (mask density, column density, run lengths) over 1 .. 3 segments: the words of the output against the
    bound for the words of the column segments that hold a selected row."""
    rng = np.random.default_rng([seed, 77])
    for draw in range(40):
        segs = int(rng.integers(1, 4))
        n = segs * SEG_WORDS
        d_mask, d_col = float(rng.choice([0.001, 0.03, 0.5, 0.97, 0.999])), float(rng.choice([0.001, 0.1, 0.5, 0.9, 0.999]))
        r_mask, r_col = float(rng.choice([1, 3, 31, 40, 500, 5000])), float(rng.choice([1, 2, 31, 62, 300, 9000]))
        mask, col = cp.words_of(_runs(rng, 32 * n, d_mask, r_mask)), cp.words_of(_runs(rng, 32 * n, d_col, r_col))
        n_rows = 32 * n - int(rng.integers(0, 2)) * int(rng.integers(0, SEG_BITS))
        delete = bool(rng.integers(0, 2))
        case = cp.Case(f"draw {seed}.{draw}", n, n_rows, n, mask, [col], delete)
        out = np.ascontiguousarray(oracle.compress(cp.model(case, 0)), dtype=np.uint32)
        bound = cp.max_words(n, 1, cp.read_source_words(oracle, case))
        assert out.size <= bound, (case.name, out.size, bound, d_mask, d_col, r_mask, r_col, n_rows, delete)


def test_the_bound_needs_two_words_per_source_word():
    """Isolated literals with bits 0 and 30 set whose survivors straddle two output groups: every literal becomes two."""
    g = np.zeros(cp.SEG_GROUPS, np.uint32)
    g[1::8] = (1 << 30) | 1
    col = _select.pack(g)
    mask = np.full(SEG_WORDS, 0xFFFFFFFF, np.uint32)
    mask[0] = 0xFFFFFFFE  # the first row goes: everything moves down by one bit
    case = cp.Case("every literal becomes two", SEG_WORDS, SEG_BITS, SEG_WORDS, mask, [col])
    out = _foreign.unpack(cp.model(case, 0))
    assert np.count_nonzero(out) == 2 * np.count_nonzero(g)


def test_named_cases_reach_what_their_names_say():
    seam = cp.seam()
    sel = seam.selected()
    assert sel.size == SEG_BITS + 5 and int(sel[SEG_BITS]) % 31 and int(sel[SEG_BITS]) % 32
    assert int(sel[SEG_BITS - 1]) // SEG_BITS == int(sel[SEG_BITS]) // SEG_BITS == 1, "source segment 1 feeds both output segments"
    assert cp.one_segment_of_rows().total_rows == SEG_BITS
    full = cp.full_output()
    assert full.total_rows == 32 * full.n_words_out and _select.pad_bits(full.n_words_out)
    assert cp.overfull_output().total_rows == 32 * full.n_words_out + 1
    seventy = cp.seventy_sources()
    assert np.array_equal(np.diff(cp.ranks(seventy)), np.ones(70)) and seventy.n_words_out == SEG_WORDS
    for delete in (False, True):
        case = cp.fill_mask_segments(delete)
        counts = np.diff(cp.ranks(case))
        assert counts[1] == (SEG_BITS if delete else 0) and counts[2] == (0 if delete else SEG_BITS) and counts[4] == 0 and counts[0] and counts[3]
        assert cp.all_ones(delete).total_rows == (0 if delete else 32 * cp.all_ones(delete).n_words)
        assert cp.all_zeros(delete).total_rows == (32 * cp.all_zeros(delete).n_words if delete else 0)
        assert cp.no_rows(delete).total_rows == 0
        assert _select.pad_bits(cp.pad_rows(delete).n_words) and cp.pad_rows(delete).n_rows == 32 * cp.pad_rows(delete).n_words
    assert cp.full_grid_columns() > cp.GRID_CAP * cp.SEG_WAVES


def test_the_grid_cap_is_the_launcher_s():
    import os
    import re

    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-wah_amd", "csrc", "wah_compact.hip")
    with open(path) as f:
        body = f.read().split("hipError_t launch_compact_segments", 1)[1]
    a, b = re.search(r"most = (\d+)u \* (\d+)u;", body).groups()
    assert int(a) * int(b) == cp.GRID_CAP


WRONG_ON = {
    "seam off by one": lambda: cp.seam(),
    "pad rows selected under DELETE": lambda: cp.pad_rows(True),
    "second destination group dropped": lambda: cp.half(),
    "carry lost between steps": lambda: cp.step_edges(),
}


@pytest.mark.parametrize("wrong", cp.WRONG_MODELS)
def test_a_wrong_model_changes_an_answer(wrong):
    case = WRONG_ON[wrong]()
    changed = int(cp.ranks(case, wrong)[-1]) != case.total_rows
    for c in range(case.n_columns):
        right = cp.arithmetic(case, c)
        assert np.array_equal(right, cp.model(case, c))
        changed |= not np.array_equal(cp.arithmetic(case, c, wrong), right)
    assert changed, wrong


def test_scratch_bytes_by_hand():
    assert cp.scratch_bytes(1, 1, 1) == 1024 + 256 + 512 + 512
    # 5000 source segments: 5001 ranks = 40 008 bytes -> 40 192, two level-1 entries; 64 x 1024 + 1 index entries: 17 level-1 entries
    assert cp.scratch_bytes(5000 * SEG_WORDS, 1024 * SEG_WORDS, 64) == 1024 + 40192 + (256 + 256) + (256 + 256)

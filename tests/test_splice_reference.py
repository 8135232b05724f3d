"""CPU proof of tests/_splice.py: the kernel's group move equals the bit-level model on every named case, every case reaches what
its name says, wah_splice_max_words holds against the reference's word counts, and the grid cap is read out of the source.  No
GPU and no library."""
import numpy as np
import pytest

from tests import _foreign, _oracle, _select, _splice as sp

SEG_BITS, SEG_WORDS, SEG_GROUPS = sp.SEG_BITS, sp.SEG_WORDS, sp.SEG_GROUPS


@pytest.fixture(scope="module")
def oracle():
    return _oracle.load()


CASES = sp.named_cases()
BY_NAME = {c.name: c for c in CASES}


def _trace(case, c=0):
    t = []
    sp.group_move(case, c, trace=t)
    return t


def test_case_names_are_unique_and_pieces_lie_inside_their_sources():
    assert len(BY_NAME) == len(CASES)
    for case in CASES:
        assert case.total_rows <= 32 * case.n_words_out, case.name
        for p, (n_words, first, n) in enumerate(case.pieces):
            assert n == 0 or first + n <= 32 * n_words, case.name
            for src in case.sources[p]:
                assert (src is None and n == 0) or src.size == n_words, case.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_group_move_equals_the_model(case):
    """... with the sources' pad bits clear and with all of them set: they die in the mask."""
    for c in range(case.n_columns):
        want = sp.model(case.column(c), case.n_words_out)
        assert np.array_equal(sp.group_move(case, c), want), (case.name, c)
        assert np.array_equal(sp.group_move(case, c, set_pad=True), want), (case.name, c, "set pad bits")


def test_group_move_equals_the_model_on_random_pieces():
    """Sources of 1, 31, 992, 993, 1984 and 2000 words of every kind, arbitrary offsets."""
    rng = np.random.default_rng(90)
    lengths = (1, 31, 992, 993, 1984, 2000)
    for trial in range(40):
        pieces, sources, rows = [], [], 0
        for _ in range(int(rng.integers(1, 6))):
            n = int(lengths[rng.integers(0, len(lengths))])
            first = int(rng.integers(0, 32 * n))
            count = int(rng.integers(0, 32 * n - first + 1))
            pieces.append((n, first, count))
            sources.append([sp.source(sp.KINDS[(trial + len(pieces)) % 4], n, trial)])
            rows += count
        n_out = (rows + 31) // 32 + int(rng.integers(0, 40)) + (rows == 0)
        case = sp.Case(f"random {trial}", n_out, pieces, sources)
        want = sp.model(case.column(0), n_out)
        assert np.array_equal(sp.group_move(case, 0, set_pad=True), want), (trial, pieces, n_out)


def test_full_grid_case_on_a_sample_of_its_columns():
    case = sp.full_grid()
    cap = sp.grid_cap()
    assert case.n_columns == cap * sp.SEG_WAVES + 1
    per = -(-case.n_columns // (cap * sp.SEG_WAVES))
    assert per == 2, "a wavefront takes a second item"
    for c in (0, 1, 2, case.n_columns // 2, case.n_columns - 1):
        assert np.array_equal(sp.group_move(case, c), sp.model(case.column(c), case.n_words_out))
    # neighbouring items differ: a wave that carried its first item's image into the second would be seen
    assert sum(np.array_equal(case.sources[0][c], case.sources[0][c + 1]) for c in range(case.n_columns - 1)) < case.n_columns // 100


def test_the_grid_cap_is_read_out_of_the_source():
    assert sp.grid_cap() == 256 * 5


# ---- every case reaches what its name says ---------------------------------------------------------------------------------------
def test_identity_cases_take_every_row_and_are_the_source(oracle):
    for n in sp.IDENTITY_WORDS:
        case = BY_NAME[f"identity {n} words"]
        assert case.total_rows == 32 * n == 32 * case.n_words_out and case.n_columns == 4
        stream, _ = sp.reference(oracle, case)
        assert np.array_equal(stream, np.concatenate([oracle.compress(s) for s in case.sources[0]]))
        assert all(q == 0 and r == 0 for _, _, _, q, r in _trace(case))


def test_identity_cases_in_foreign_ways_differ_from_the_canonical_stream(oracle):
    for n in sp.IDENTITY_WORDS:
        for way in _foreign.ways_for(n)[1:]:
            case = sp.identity(n, way)
            changed = 0
            for c in range(case.n_columns):
                st = case.stream_of(oracle, 0, c)
                assert np.array_equal(oracle.decompress(st)[:n], case.sources[0][c]), (n, way, c)
                changed += not np.array_equal(st, oracle.compress(case.sources[0][c]))
            assert changed or (n == 1 and way not in _foreign.PAD_WAYS), (n, way)  # (two groups: little to rewrite)


def test_shift_sweep_reaches_its_shifts():
    rs, qs, two = set(), set(), 0
    for f in sp.SHIFTS:
        t = _trace(BY_NAME[f"shift {f}"])
        rs |= {r for *_, r in t}
        qs |= {q for *_, q, _ in t}
        two += len({ss for _, _, ss, _, _ in t}) == 2
    assert {0, 1, 30} <= rs and max(qs) == 1023 and min(qs) <= -1, (rs, qs)
    assert two >= 6, "two source segments for one output segment"


def test_front_pieces_give_negative_deltas():
    for b in sp.FRONTS:
        t = _trace(BY_NAME[f"front {b}"])
        second = [(q, r) for _, p, _, q, r in t if p == 1]
        assert second == [(-((b + 30) // 31), (-b) % 31)], (b, second)


def test_piece_edge_cases():
    case = BY_NAME["65 pieces of one row"]
    assert len(case.pieces) == 65 and all(n == 1 for _, _, n in case.pieces) and _select.segments_of(case.n_words_out) == 1
    assert len({s.tobytes() for row in case.sources for s in row}) > 65
    assert [n for _, _, n in BY_NAME["pieces of 30, 31 and 32 rows"].pieces] == [30, 31, 32, 30, 31, 32]
    case = BY_NAME["a piece ending on a segment edge"]
    assert case.pieces[0][2] == SEG_BITS and {(seg, p) for seg, p, *_ in _trace(case)} == {(0, 0), (1, 1)}
    case = BY_NAME["a piece across an output edge and a source edge"]
    t = [(seg, ss) for seg, p, ss, _, _ in _trace(case) if p == 1]
    assert t == [(0, 0), (0, 1), (1, 1)], t


def test_runs_of_ones(oracle):
    stream, index = sp.reference(oracle, BY_NAME["two runs of ones: one fill"])
    assert stream.tolist() == [sp.FILL1 | SEG_GROUPS] and index.tolist() == [0, 1]
    stream, _ = sp.reference(oracle, BY_NAME["ones across a segment edge: two fills"])
    assert stream.tolist() == [sp.FILL1 | SEG_GROUPS] * 2
    stream, _ = sp.reference(oracle, BY_NAME["ones ending inside a group"])
    full, rest = divmod(1100, 31)
    assert stream.tolist() == [sp.FILL1 | full, (1 << rest) - 1, sp.FILL0 | (SEG_GROUPS - full - 1)]  # ... and the tail behind T


def test_ragged_cases(oracle):
    case = BY_NAME["the last rows of ragged sources"]
    assert [first + n for (_, first, n) in case.pieces] == [32, 32 * 31, 32 * 993]
    for n in (1, 993, 1000):
        assert BY_NAME[f"{n} words out"].n_words_out == n
    case = BY_NAME["T fills a ragged output"]
    assert case.total_rows == 32 * case.n_words_out and _select.pad_bits(case.n_words_out) > 0
    stream, _ = sp.reference(oracle, case)
    assert stream[:2].tolist() == [sp.FILL1 | SEG_GROUPS, sp.FILL1 | 1] and stream[2] == 1  # column 0: all ones, pad bits clear
    case = BY_NAME["no rows at all"]
    assert case.total_rows == 0 and all(s is None for row in case.sources for s in row)
    stream, _ = sp.reference(oracle, case)
    assert stream.tolist() == [sp.FILL0 | SEG_GROUPS, sp.FILL0 | 2] * 2
    for way in _foreign.PAD_WAYS:
        case = sp.pad_tail(way)
        st = case.stream_of(oracle, 0, 0)
        assert _select.stream_count(st, 993) == 32 * 993 and not np.array_equal(st, oracle.compress(case.sources[0][0]))
        assert case.pieces[0][1] + case.pieces[0][2] == 32 * 993 and case.total_rows < 32 * case.n_words_out
        got = sp.model(case.column(0), case.n_words_out)
        assert sp.bits_of(got).sum() == 500


def test_column_cases(oracle):
    case = BY_NAME["3 columns x 2 pieces"]
    assert case.n_columns == 3 and len(case.pieces) == 2
    assert len({s.tobytes() for row in case.sources for s in row}) == 6
    # the table read piece-major with the roles swapped is another result
    assert not np.array_equal(sp.model(case.column(0), case.n_words_out), sp.model(case.column(1), case.n_words_out))
    case = BY_NAME["one more segment than a workgroup has waves"]
    assert _select.segments_of(case.n_words_out) == sp.SEG_WAVES + 1 and case.n_columns == 1


# ---- the size bound ------------------------------------------------------------------------------------------------------------
def _bound_terms(oracle, case):
    stream, _ = sp.reference(oracle, case)
    touched = sp.touched_source_words(oracle, case)
    return stream.size, touched


@pytest.mark.parametrize("case", CASES + [sp.pad_tail(w) for w in _foreign.PAD_WAYS[1:]], ids=lambda c: c.name)
def test_max_words_holds(oracle, case):
    words, touched = _bound_terms(oracle, case)
    assert words <= sp.max_words(case.n_words_out, case.n_columns, len(case.pieces), touched), (case.name, words, touched)


def test_max_words_holds_on_the_full_grid_case(oracle):
    case = sp.full_grid()
    words, touched = _bound_terms(oracle, case)
    assert words <= sp.max_words(case.n_words_out, case.n_columns, 1, touched)


def test_max_words_needs_both_of_its_arms(oracle):
    case = BY_NAME["every literal becomes two"]
    words, touched = _bound_terms(oracle, case)
    s = _select.segments_of(case.n_words_out)
    without_the_two = case.n_columns * (s + 1) + 2 * len(case.pieces) * case.n_columns + touched
    assert without_the_two < words <= sp.max_words(case.n_words_out, 1, 1, touched) < _select.groups_of(case.n_words_out)
    case = BY_NAME["dense: the groups bound"]
    words, touched = _bound_terms(oracle, case)
    g = _select.groups_of(case.n_words_out)
    assert sp.max_words(case.n_words_out, 2, 1, touched) == 2 * g < 2 * (s + 1) + 4 + 2 * touched and words > 2 * g - 8


def test_max_words_against_adversarial_pieces(oracle):
    """Alternating literals and fills cut at every offset of a group, many pieces: the per-piece and per-literal terms."""
    rng = np.random.default_rng(91)
    g = np.zeros(SEG_GROUPS, np.uint32)
    g[::2] = (1 << 30) | 1
    lit = _select.pack(g)
    ones = np.full(SEG_WORDS, 0xFFFFFFFF, np.uint32)
    for trial in range(12):
        pieces, sources, rows = [], [], 0
        while rows < SEG_BITS - 700:
            n = int(rng.integers(1, 700))
            first = int(rng.integers(0, SEG_BITS - n))
            pieces.append((SEG_WORDS, first, n))
            sources.append([lit if (len(pieces) + trial) % 2 else ones])
            rows += n
        case = sp.Case(f"adversarial {trial}", SEG_WORDS, pieces, sources)
        words, touched = _bound_terms(oracle, case)
        # the bound with the words of the touched source segments, and with the tighter count of the words a piece's range meets
        assert words <= sp.max_words(SEG_WORDS, 1, len(pieces), touched), (trial, words)
        assert words <= sp.max_words(SEG_WORDS, 1, len(pieces), sp.met_source_words(oracle, case)), (trial, words)

"""CPU tests of the partitioned running-sum tests' own reference (tests/_cumsum_parts.py): the value model, its slice matrix through
the oracle's compress() and the restatement of the kernels' steps agree on every named case and on random draws, every wrong model
changes the answer of the named case that is meant to catch it, an empty starts bitmap gives tests/_cumsum.py's model, the scan's
round seam carries a pair, and the constants the tests state are the ones in csrc/wah_cumsum.hip."""
import os
import re

import numpy as np
import pytest

from tests import _bsi, _cumsum as cs, _cumsum_parts as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return cp.named_cases()


@pytest.fixture(scope="module")
def answers(cases):
    """The model's answer of every named case, computed once."""
    return {name: cp.expected(case) for name, case in cases.items()}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def test_named_cases_cover_what_the_interface_names(cases):
    for kv in cp.VAL_WIDTHS:
        for k_out in cp.OUT_WIDTHS:
            assert any(c["kv"] == kv and c["k_out"] == k_out for c in cases.values()), (kv, k_out)
    for with_exists in (False, True):
        for exclusive, all_rows in cp.MODES:
            assert any((c["exists"] is not None) == with_exists and c["exclusive"] == exclusive and c["all_rows"] == all_rows and c["kv"] and c["filters"]
                       and c["starts"].any() for c in cases.values()), (with_exists, exclusive, all_rows)
    assert {len(c["filters"]) for c in cases.values()} >= {0, 1, cs.MAX_FILTERS}
    assert {c["n"] for c in cases.values()} == set(cp.SIZES)
    assert set(cp.CAUGHT_BY) == set(cp.WRONG) and len(cp.WRONG) == 7
    # the placements: the seams, lanes 0 and 63 of one step, a start at an unselected row, starts at and behind n_rows
    seams = cases["starts at the seams"]["starts"]
    assert all(seams[r] for r in (63, 64, 65, 2047, 2048, 16383, 16384, 30720, 31743, 31744))
    two = np.flatnonzero(cases["two starts in a step"]["starts"])
    assert two[0] % 64 == 0 and two[1] == two[0] + 63
    three = np.flatnonzero(cases["three starts in a step"]["starts"])
    assert three[0] % 64 == 0 and three[2] == three[0] + 63 and three[0] < three[1] < three[2]
    c = cases["starts at unselected rows"]
    assert c["starts"].any() and not (c["starts"] & cs.selection(c)).any()
    c = cases["starts at and behind n_rows"]
    assert c["starts"][c["n_rows"]] and c["starts"][c["n_rows"] + 1] and c["starts"][c["n_rows"] - 1] and c["starts"][c["n_rows"]:].sum() >= 4
    c = cases["a start in segment 0, segment 1 empty"]
    assert np.flatnonzero(c["starts"]).tolist() == [100] and not cs.selection(c)[cp.SEG_BITS: 2 * cp.SEG_BITS].any() and c["n"] == 3 * cp.SEG_WORDS
    c = cases["a start in segment 1 only"]
    assert not c["starts"][: cp.SEG_BITS].any() and c["starts"][cp.SEG_BITS: 2 * cp.SEG_BITS].sum() == 1 and not c["starts"][2 * cp.SEG_BITS:].any()
    run, _ = cp.values_of(dict(cases["partition sums past 2^32"], k_out=64))
    assert int(run.max()) > 1 << 40


def test_the_three_statements_agree_on_the_named_cases(oracle, cases, answers):
    for name, case in cases.items():
        matrix = answers[name]
        assert matrix.shape == (cp.rows_out(case), case["n"]), name
        assert _same(cp.kernel(case), matrix), name
        stream, index = cp.compressed(oracle, matrix)
        assert index.size == matrix.shape[0] * (case["n"] // cp.SEG_WORDS) + 1 and index[0] == 0 and index[-1] == stream.size, name
        assert np.array_equal(np.asarray(oracle.decompress(stream))[: matrix.size], matrix.reshape(-1)), name
        values, exists = _bsi.values_of_slices(matrix, case["k_out"])
        want, sel = cp.values_of(case)
        assert np.array_equal(values, want) and (exists is None) == case["all_rows"] and (exists is None or np.array_equal(exists, sel)), name


def test_the_model_against_a_loop():
    """The value model against a row-by-row loop in Python ints."""
    case = cp.make_case(cp.SEG_WORDS, 9, 20, 1 / 40, n_rows=5000, n_filters=1, seed=21)
    case["starts"][[0, 4999, 5000]] = True
    for exclusive in (False, True):
        for all_rows in (False, True):
            c = dict(case, exclusive=exclusive, all_rows=all_rows)
            got, sel = cp.values_of(c)
            run = 0
            for p in range(5200):
                if p < 5000 and c["starts"][p]:
                    run = 0
                x = int(c["values"][p]) if sel[p] else 0
                want = run if exclusive else run + x
                run += x
                if p >= 5000 or not (sel[p] or all_rows):
                    want = 0
                assert int(got[p]) == want % (1 << 20), (exclusive, all_rows, p)


def test_an_empty_starts_bitmap_is_the_plain_call(cases):
    for name, case in cs.named_cases().items():
        with_starts = dict(case, starts=np.zeros(32 * case["n"], bool))
        assert _same(cp.expected(with_starts), cs.expected(case)), name
    for name in ("no start, 1 segments", "no start, 2 segments", "no start, 3 segments"):
        assert not cases[name]["starts"].any() and _same(cp.expected(cases[name]), cs.expected(cases[name])), name
    behind = cases["starts at and behind n_rows"]
    cut = dict(behind, starts=behind["starts"] & (np.arange(behind["starts"].size) < behind["n_rows"]))
    assert _same(cp.expected(behind), cp.expected(cut))


def test_the_scan_carries_a_pair_over_its_round_seam():
    """8194 records with starts in 8190 .. 8193: what flows into a segment is the fold of every record in front of it."""
    rng = np.random.default_rng(8194)
    records = [(8190 <= i or i == 17, int(rng.integers(0, 1 << 62))) for i in range(8194)]
    got = cp.scan_records(records)
    run = 0
    for i, (has, total) in enumerate(records):
        assert got[i] == run, i
        run = total if has else (run + total) % (1 << 64)
    lost = list(records)
    lost[8191] = (False, records[8191][1])  # the carry of round 0 is a pair: its flag alone does not reach round 1's entries
    assert cp.scan_records(lost)[8192] == (records[8190][1] + records[8191][1]) % (1 << 64)


@pytest.mark.parametrize("n_rows_back", (0, 70, cp.SEG_BITS, 5 * cp.SEG_BITS + 9))
def test_the_long_model_is_the_dense_one_on_a_short_bitmap(oracle, n_rows_back, a=40):
    """long_expected, which the GPU tests of 8194 segments and of more than 2^32 rows are held against, on 40 segments: the stream
    and the index of the dense model."""
    from tests import _long as lg

    n_rows = a * cp.SEG_BITS - n_rows_back
    named = (0, 7, 8, 20, 33, 34, 39)
    filt = lg.marked(a, named, (0,), 5, default=1)
    at = [7 * cp.SEG_BITS + 5, 8 * cp.SEG_BITS, 20 * cp.SEG_BITS + 31743, 33 * cp.SEG_BITS + 64, 34 * cp.SEG_BITS + 1, 39 * cp.SEG_BITS + 12, a * cp.SEG_BITS - 3]
    starts = lg.from_rows(a, at)
    want, index, incoming = cp.long_expected(oracle, filt, starts, n_rows)
    case = dict(n=a * cp.SEG_WORDS, n_rows=n_rows, kv=0, values=np.zeros(32 * a * cp.SEG_WORDS, np.uint64), exists=None,
                filters=[_bsi.unpack_bits(filt.decoded())], k_out=2, exclusive=False, all_rows=True, starts=_bsi.unpack_bits(starts.decoded()))
    stream, dense_index = cp.compressed(oracle, cp.expected(case))
    assert np.array_equal(index, dense_index) and np.array_equal(want.view(np.uint32), stream)
    assert incoming[8] < cp.SEG_BITS and incoming[20] > 11 * cp.SEG_BITS


@pytest.mark.parametrize("seed", range(16))
def test_the_three_statements_agree_on_random_draws(oracle, seed):
    case = cp.random_case(seed)
    matrix = cp.expected(case)
    assert _same(cp.kernel(case), matrix), seed
    stream, index = cp.compressed(oracle, matrix)
    assert np.array_equal(np.asarray(oracle.decompress(stream))[: matrix.size], matrix.reshape(-1)) and index[-1] == stream.size, seed


@pytest.mark.parametrize("wrong", cp.WRONG)
def test_every_wrong_model_is_caught(cases, answers, wrong):
    name = cp.CAUGHT_BY[wrong]
    assert not _same(cp.kernel(cases[name], wrong), answers[name]), (wrong, name)


def test_the_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_cumsum.hip")).read()
    assert re.search(r"constexpr u32 kScanWaves = 16;", text) and re.search(r"constexpr u32 kScanPer = 8;", text) and cp.SCAN_ROUND == 16 * 64 * 8
    assert re.search(r"constexpr u32 kPartsSliceWaves = kCumsumWaves - 2u;", text)
    assert "cumsum_parts_totals_kernel" in text and "cumsum_parts_scan_kernel" in text and "cumsum_parts_rows_kernel" in text

"""CPU tests of the partition-total tests' own reference (tests/_total_parts.py): the value model, its slice matrix through the oracle's
compress() and the restatement of the kernels' steps agree on every named case and on random draws, every wrong model changes the
answer of the named case that is meant to catch it, the total is the partitioned running sum at the partition's last row, every row
a start gives the selected value itself and no start the grand total, both scans carry a pair over their round seams, the long
model is the dense one, and the constants the tests state are the ones in csrc/wah_cumsum.hip."""
import os
import re

import numpy as np
import pytest

from tests import _bsi, _cumsum as cs, _cumsum_parts as cp, _total_parts as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return tp.named_cases()


@pytest.fixture(scope="module")
def answers(cases):
    """The model's answer of every named case, computed once."""
    return {name: tp.expected(case) for name, case in cases.items()}


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def test_named_cases_cover_what_the_interface_names(cases):
    for kv in tp.VAL_WIDTHS:
        for k_out in tp.OUT_WIDTHS:
            assert any(c["kv"] == kv and c["k_out"] == k_out for c in cases.values()), (kv, k_out)
    for with_exists in (False, True):
        for all_rows in (False, True):
            assert any((c["exists"] is not None) == with_exists and c["all_rows"] == all_rows and c["kv"] and c["filters"] and c["starts"].any()
                       for c in cases.values()), (with_exists, all_rows)
    assert not any(c["exclusive"] for c in cases.values())
    assert {len(c["filters"]) for c in cases.values()} >= {0, 1, cs.MAX_FILTERS}
    assert {c["n"] for c in cases.values()} == set(tp.SIZES)
    assert set(tp.CAUGHT_BY) == set(tp.WRONG) and len(tp.WRONG) == 7
    seams = (63, 64, 65, 2047, 2048, 16383, 16384, 30720, 31743, 31744)
    assert tp.SEAMS == seams and all(cases["starts at the seams"]["starts"][[r, tp.SEG_BITS + r]].all() for r in seams)
    for r in seams + tuple(tp.SEG_BITS + r for r in seams):
        assert np.flatnonzero(cases[f"a start at row {r} alone"]["starts"]).tolist() == [r]
    two = np.flatnonzero(cases["two starts in a step"]["starts"])
    assert two[0] % 64 == 0 and two[1] == two[0] + 63
    three = np.flatnonzero(cases["three starts in a step"]["starts"])
    assert three[0] % 64 == 0 and three[2] == three[0] + 63 and three[0] < three[1] < three[2]
    c = cases["starts at a block's, a segment's and the table's ends"]
    at = np.flatnonzero(c["starts"])
    assert at[0] % tp.BLOCK_ROWS == 0 and at[1] == tp.SEG_BITS and at[-1] == c["n_rows"] - 1
    c = cases["starts at unselected rows"]
    assert c["starts"].any() and not (c["starts"] & cs.selection(c)).any()
    c = cases["starts at and behind n_rows"]
    assert c["starts"][c["n_rows"]] and c["starts"][c["n_rows"] + 1] and c["starts"][c["n_rows"] - 1] and c["starts"][c["n_rows"]:].sum() >= 4
    for name, selected in (("a partition over three segments", True), ("a partition over three segments, the middle one empty", False)):
        c = cases[name]
        assert np.flatnonzero(c["starts"]).tolist() == [100] and c["n"] == 3 * tp.SEG_WORDS
        assert cs.selection(c)[tp.SEG_BITS: 2 * tp.SEG_BITS].any() == selected
    c = cases["a partition without a selected row all_rows"]
    values, sel = tp.values_of(c)
    assert not sel[5000:9000].any() and not values[5000:9000].any() and values[4999] and values[9000]
    total, _ = tp.values_of(dict(cases["totals past 2^32"], k_out=64))
    assert int(total.max()) > 1 << 40
    total, _ = tp.values_of(dict(cases["totals past 2^32 truncated"], k_out=64))
    assert int(total.max()) >> 33


def test_the_three_statements_agree_on_the_named_cases(oracle, cases, answers):
    for name, case in cases.items():
        matrix = answers[name]
        assert matrix.shape == (tp.rows_out(case), case["n"]), name
        assert _same(tp.kernel(case), matrix), name
        stream, index = tp.compressed(oracle, matrix)
        assert index.size == matrix.shape[0] * (case["n"] // tp.SEG_WORDS) + 1 and index[0] == 0 and index[-1] == stream.size, name
        assert np.array_equal(np.asarray(oracle.decompress(stream))[: matrix.size], matrix.reshape(-1)), name
        values, exists = _bsi.values_of_slices(matrix, case["k_out"])
        want, sel = tp.values_of(case)
        assert np.array_equal(values, want) and (exists is None) == case["all_rows"] and (exists is None or np.array_equal(exists, sel)), name


def test_the_model_against_a_loop():
    """The value model against a row-by-row loop in Python ints."""
    case = tp.make_case(tp.SEG_WORDS, 9, 20, 1 / 40, n_rows=5000, n_filters=1, seed=21)
    case["starts"][[0, 4999, 5000]] = True
    for all_rows in (False, True):
        c = dict(case, all_rows=all_rows)
        got, sel = tp.values_of(c)
        p = 0
        while p < 5000:
            q = p + 1
            while q < 5000 and not c["starts"][q]:
                q += 1
            total = sum(int(c["values"][i]) for i in range(p, q) if sel[i])
            for i in range(p, q):
                assert int(got[i]) == (total % (1 << 20) if sel[i] or all_rows else 0), (all_rows, i)
            p = q
        assert not got[5000:].any()


def test_the_total_is_the_running_sum_at_the_partitions_last_row(cases):
    """T under all_rows is tests/_cumsum_parts.py's inclusive all_rows value at e(p), the row in front of the next start (n_rows - 1
    in the last partition)."""
    for name, case in cases.items():
        if case["n_rows"] == 0:
            continue
        c = dict(case, all_rows=True)
        running, _ = cp.values_of(c)
        st = tp.effective_starts(c)
        rows = st.size
        nxt = np.where(st, np.arange(rows), rows)
        nxt = np.minimum.accumulate(nxt[::-1])[::-1]          # the first start at or behind a row
        end = np.concatenate([nxt[1:], [rows]]) - 1             # e(p): the row in front of the first start behind it
        end = np.minimum(end, c["n_rows"] - 1)
        total, _ = tp.values_of(c)
        p = np.arange(c["n_rows"])
        assert np.array_equal(total[p], running[end[p]]), name


def test_every_row_a_start_and_no_start(cases):
    for i in (1, 2, 3):
        c = cases[f"every row a start, {i} segments"]
        values, sel = tp.values_of(c)
        assert np.array_equal(values, np.where(sel, c["values"], 0) & np.uint64((1 << c["k_out"]) - 1))
        c = cases[f"no start, {i} segments"]
        values, sel = tp.values_of(c)
        grand = int(np.where(sel, c["values"], 0).sum(dtype=np.uint64)) % (1 << c["k_out"])
        keep = (np.arange(sel.size) < c["n_rows"]) if c["all_rows"] else sel
        assert grand and np.array_equal(values, np.where(keep, np.uint64(grand), np.uint64(0)))
    behind = cases["starts at and behind n_rows"]
    cut = dict(behind, starts=behind["starts"] & (np.arange(behind["starts"].size) < behind["n_rows"]))
    assert _same(tp.expected(behind), tp.expected(cut))


def _brute_scans(records):
    n = len(records)
    forward, run = [], 0
    for f, _, t in records:
        forward.append(run)
        run = t if f else (run + t) % (1 << 64)
    backward = [0] * n
    for i in range(n):
        total = 0
        for f, h, _ in records[i + 1:]:
            total = (total + h) % (1 << 64)
            if f:
                break
        backward[i] = total
    return forward, backward


def test_both_scans_carry_a_pair_over_their_round_seams():
    """8194 records with starts in the first four and the last four: the forward round seam lies behind record 8191, the backward one
    in front of record 2, and the wrong model that loses the backward carry of the short last round changes what flows into
    record 1."""
    records = tp.round_seam_records()
    assert len(records) == tp.SCAN_ROUND + 2 and [i for i, r in enumerate(records) if r[0]] == [0, 1, 2, 3, 8190, 8191, 8192, 8193]
    forward, backward = tp.scan_records(records)
    run = 0
    for i, (f, _, t) in enumerate(records):
        assert forward[i] == run, i
        run = t if f else (run + t) % (1 << 64)
    run = 0
    for i in range(len(records) - 1, -1, -1):
        assert backward[i] == run, i
        f, h, _ = records[i]
        run = h if f else (run + h) % (1 << 64)
    assert backward[1] == records[2][1] and backward[0] == records[1][1]
    small = [(bool(i % 3 == 0), i * 7 + 1, i * 11 + 2) for i in range(40)]
    assert tp.scan_records(small) == _brute_scans(small)
    lost = tp.scan_records(records, tp.WRONG[5])
    assert lost[0] == forward and lost[1][2:] == backward[2:] and lost[1][1] == 0 != backward[1]
    # the carry is a pair: without record 8190's flag the backward inflow of 8189 is still cut at 8191
    middle = list(records)
    middle[8190] = (False,) + records[8190][1:]
    assert tp.scan_records(middle)[1][8189] == (records[8190][1] + records[8191][1]) % (1 << 64)


@pytest.mark.parametrize("n_rows_back", (0, 70, tp.SEG_BITS, 5 * tp.SEG_BITS + 9))
def test_the_long_model_is_the_dense_one_on_a_short_bitmap(oracle, n_rows_back, a=40):
    """long_expected, which the GPU tests of 8194 segments and of more than 2^32 rows are held against, on 40 segments: the stream
    and the index of the dense model."""
    from tests import _long as lg

    n_rows = a * tp.SEG_BITS - n_rows_back
    named = (0, 7, 8, 20, 33, 34, 39)
    filt = lg.marked(a, named, (0,), 5, default=1)
    at = [7 * tp.SEG_BITS + 5, 8 * tp.SEG_BITS, 20 * tp.SEG_BITS + 31743, 33 * tp.SEG_BITS + 64, 34 * tp.SEG_BITS + 1, 39 * tp.SEG_BITS + 12, a * tp.SEG_BITS - 3]
    starts = lg.from_rows(a, at)
    want, index, sizes = tp.long_expected(oracle, filt, starts, n_rows)
    case = dict(n=a * tp.SEG_WORDS, n_rows=n_rows, kv=0, values=np.zeros(32 * a * tp.SEG_WORDS, np.uint64), exists=None,
                filters=[_bsi.unpack_bits(filt.decoded())], k_out=2, exclusive=False, all_rows=True, starts=_bsi.unpack_bits(starts.decoded()))
    stream, dense_index = tp.compressed(oracle, tp.expected(case))
    assert np.array_equal(index, dense_index) and np.array_equal(want.view(np.uint32), stream)
    assert sizes.size == int(tp.effective_starts(case).sum()) + 1 and int(sizes.max()) > 11 * tp.SEG_BITS


@pytest.mark.parametrize("seed", range(16))
def test_the_three_statements_agree_on_random_draws(oracle, seed):
    case = tp.random_case(seed)
    matrix = tp.expected(case)
    assert _same(tp.kernel(case), matrix), seed
    stream, index = tp.compressed(oracle, matrix)
    assert np.array_equal(np.asarray(oracle.decompress(stream))[: matrix.size], matrix.reshape(-1)) and index[-1] == stream.size, seed


@pytest.mark.parametrize("wrong", tp.WRONG)
def test_every_wrong_model_is_caught(cases, answers, wrong):
    name = tp.CAUGHT_BY[wrong]
    if name == "records":
        records = tp.round_seam_records()
        assert tp.scan_records(records, wrong) != tp.scan_records(records), wrong
        return
    assert not _same(tp.kernel(cases[name], wrong), answers[name]), (wrong, name)


def test_the_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_cumsum.hip")).read()
    assert re.search(r"constexpr u32 kScanWaves = 16;", text) and re.search(r"constexpr u32 kScanPer = 8;", text) and tp.SCAN_ROUND == 16 * 64 * 8
    assert "total_parts_records_kernel" in text and "total_parts_scan_kernel" in text and "total_parts_rows_kernel" in text
    header = open(os.path.join(ROOT, "gpu-wah_amd", "csrc", "wah_internal.hpp")).read()
    fields = re.search(r"struct BsiTotalPartsRecord \{(.*?)\};", header, re.S).group(1)
    assert len(re.findall(r"uint64_t \w+;", fields)) * 8 == tp.RECORD_BYTES

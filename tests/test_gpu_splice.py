"""GPU tests of wah_splice_indexed_device (include/wah.h) and its front ends: row ranges of indexed bitmaps concatenated into new
indexed bitmaps.  Everything is exact: the words, their count and every index entry against the CPU oracle's compress() of the
bit-level concatenation (tests/_splice.py: model, reference).  tests/test_splice_reference.py proves on the CPU that every named
case reaches what its name says.  The largest output is five segments; the widest call has one column more than four grids."""
import importlib

import numpy as np
import pytest

from tests import _foreign, _select, _splice as sp

pytestmark = pytest.mark.gpu

WAH_OK, WAH_ERR_CAPACITY, WAH_ERR_STREAM = 0, -4, -6
SEG_WORDS, SEG_BITS = sp.SEG_WORDS, sp.SEG_BITS
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def wah():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    pkg = importlib.import_module("gpu-wah_amd")
    pkg.lib()  # raises if the HIP extension is missing: no fallback
    return pkg


def _host(t):
    return t.cpu().numpy().view(np.uint32)


class Operands:
    """The sources of a case in device memory: one buffer of all streams, one of all indexes, and the [n_pieces * n_columns, 3]
    table over them, piece-major; a source that is None is a null entry.  rows: (first word, words, first index entry) per entry."""

    def __init__(self, oracle, case, streams=None):
        import torch

        words, entries, self.rows = [], [], []
        at = at_index = 0
        for p in range(len(case.pieces)):
            for c in range(case.n_columns):
                if case.sources[p][c] is None:
                    self.rows.append(None)
                    continue
                st, idx = streams[(p, c)] if streams and (p, c) in streams else (case.stream_of(oracle, p, c), None)
                idx = _select.index_of(st) if idx is None else idx
                assert idx.size == _select.segments_of(case.pieces[p][0]) + 1, (case.name, p, c)
                self.rows.append((at, st.size, at_index))
                words.append(st)
                entries.append(idx)
                at, at_index = at + st.size, at_index + idx.size
        self.stream = torch.from_numpy(np.concatenate(words + [np.zeros(1, np.uint32)]).view(np.int32)).cuda()
        self.index = torch.from_numpy(np.concatenate(entries + [np.zeros(1, np.int64)])).cuda()
        self.table = torch.tensor(self.host_table(), dtype=torch.int64, device="cuda")
        self.pieces = torch.tensor(case.pieces, dtype=torch.int64, device="cuda")

    def host_table(self, order=None):
        rows = [(0, 0, 0) if r is None else (self.stream.data_ptr() + 4 * r[0], r[1], self.index.data_ptr() + 8 * r[2]) for r in self.rows]
        return rows if order is None else [rows[i] for i in order]


def _run(wah, case, ops, **kw):
    return wah.splice_device(ops.pieces, ops.table, case.n_columns, case.n_words_out, **kw)


def _check(case, got, want, what=None):
    stream, offs = got
    want_stream, want_index = want
    what = what or case.name
    assert stream.numel() == want_stream.size, (what, stream.numel(), want_stream.size)
    assert np.array_equal(_host(stream), want_stream), what
    assert offs.numel() == want_index.size and np.array_equal(offs.cpu().numpy(), want_index), what


def _run_guarded(wah, oracle, case, ops=None):
    """The call into an output of exactly wah_splice_max_words words for the touched source segments, a guard word behind it."""
    import torch

    ops = ops or Operands(oracle, case)
    cap = wah.splice_max_words(case.n_words_out, case.n_columns, len(case.pieces), sp.touched_source_words(oracle, case))
    buf = torch.full((cap + 1,), GUARD, dtype=torch.int32, device="cuda")
    got = _run(wah, case, ops, out=buf[:cap])
    assert int(buf[cap].item()) == GUARD, case.name
    return got


# ---- 1 .. 6: the named cases -------------------------------------------------------------------------------------------------------
CASES = sp.named_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_named_case(wah, oracle, case):
    _check(case, _run_guarded(wah, oracle, case), sp.reference(oracle, case))


FOREIGN = [(n, way) for n in sp.IDENTITY_WORDS for way in _foreign.ways_for(n)[1:]]


@pytest.mark.parametrize("n,way", FOREIGN, ids=[f"{n}-{way}" for n, way in FOREIGN])
def test_identity_of_a_foreign_stream_is_the_canonical_stream(wah, oracle, n, way):
    case = sp.identity(n, way)
    got = _run_guarded(wah, oracle, case)
    _check(case, got, sp.reference(oracle, case))
    assert np.array_equal(_host(got[0]), np.concatenate([oracle.compress(s) for s in case.sources[0]])), case.name


@pytest.mark.parametrize("way", _foreign.PAD_WAYS)
def test_set_pad_bits_in_front_of_the_tail(wah, oracle, way):
    case = sp.pad_tail(way)
    _check(case, _run_guarded(wah, oracle, case), sp.reference(oracle, case))


def test_a_transposed_table_is_another_result(wah, oracle):
    import torch

    case = next(c for c in CASES if c.name == "3 columns x 2 pieces")
    ops = Operands(oracle, case)
    want = sp.reference(oracle, case)
    _check(case, _run(wah, case, ops), want)
    p, k = len(case.pieces), case.n_columns
    ops.table = torch.tensor(ops.host_table([i % p * k + i // p for i in range(p * k)]), dtype=torch.int64, device="cuda")  # column-major
    got = _run(wah, case, ops)  # (all six sources are as long as their pieces say: legal, and another bitmap)
    assert got[0].numel() != want[0].size or not np.array_equal(_host(got[0]), want[0])


def test_a_wavefront_takes_a_second_item(wah, oracle):
    case = sp.full_grid()
    ops = Operands(oracle, case)
    _check(case, _run(wah, case, ops), sp.reference(oracle, case))


# ---- 7: the front ends ---------------------------------------------------------------------------------------------------------------
def _dev_i64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


ROW_COUNTS = ((1000, SEG_BITS), (SEG_BITS, 5))


@pytest.mark.parametrize("rows,batch_rows", ROW_COUNTS)
def test_append_rows_of_an_equality_encoded_index(wah, rows, batch_rows):
    import torch

    n_values = 7
    keys = np.random.default_rng([rows, batch_rows]).integers(0, n_values, rows + batch_rows)
    index = wah.columns.index_from_keys(wah, _dev_i64(keys[:rows]), n_values)
    batch = wah.columns.index_from_keys(wah, _dev_i64(keys[rows:]), n_values)
    both = wah.columns.append_rows(wah, index, rows, batch, batch_rows)
    assert len(both) == 3 and both[2] == 2 * SEG_WORDS and both[1].numel() == n_values * 2 + 1
    every = torch.arange(32 * both[2], dtype=torch.int64, device="cuda")
    got = wah.columns.keys_at_rows(wah, both, every).cpu().numpy()
    assert np.array_equal(got[: keys.size], keys) and bool((got[keys.size:] == -1).all())
    # the result goes unchanged into the calls that read an index
    counts = wah.columns.count_columns(wah, *both, list(range(n_values))).cpu().numpy()
    assert np.array_equal(counts, np.bincount(keys, minlength=n_values))
    whole = wah.columns.index_from_keys(wah, _dev_i64(keys), n_values)
    assert both[0].numel() == whole[0].numel() and bool((both[0] == whole[0]).all()) and bool((both[1] == whole[1]).all())


@pytest.mark.parametrize("rows,batch_rows", ROW_COUNTS)
def test_append_and_slice_rows_of_a_bit_sliced_index(wah, rows, batch_rows):
    import torch

    n_bits = 20
    rng = np.random.default_rng([rows, batch_rows, 1])
    values = rng.integers(0, 1 << n_bits, rows + batch_rows)
    exists = rng.random(values.size) < 0.8
    d_exists = torch.from_numpy(exists).cuda()
    index = wah.columns.bsi_from_values(wah, _dev_i64(values[:rows]), n_bits, exists=d_exists[:rows].clone())
    batch = wah.columns.bsi_from_values(wah, _dev_i64(values[rows:]), n_bits, exists=d_exists[rows:].clone())
    both = wah.columns.append_rows(wah, index, rows, batch, batch_rows)
    assert len(both) == 5 and both[2:] == (2 * SEG_WORDS, n_bits, True)
    every = torch.arange(values.size, dtype=torch.int64, device="cuda")
    got, have = wah.columns.values_at_rows(wah, both, every)
    assert np.array_equal(have.cpu().numpy(), exists) and np.array_equal(got.cpu().numpy(), np.where(exists, values, 0))
    # ... and into range_column
    lo, hi = 1 << 17, 3 << 17
    stream, offs = wah.columns.range_column(wah, both, lo, hi)
    positions, total = wah.positions_device(stream, offs, both[2])
    want = np.flatnonzero(exists & (values >= lo) & (values <= hi))
    assert total == want.size and np.array_equal(positions.cpu().numpy(), want)
    # a window of it
    first, n = 977, min(values.size - 977, SEG_BITS + 40)
    part = wah.columns.slice_rows(wah, both, first, n)
    assert len(part) == 5 and part[3:] == (n_bits, True) and part[2] == -(-((n + 31) // 32) // SEG_WORDS) * SEG_WORDS
    got, have = wah.columns.values_at_rows(wah, part, torch.arange(n, dtype=torch.int64, device="cuda"))
    assert np.array_equal(have.cpu().numpy(), exists[first: first + n])
    assert np.array_equal(got.cpu().numpy(), np.where(exists, values, 0)[first: first + n])
    behind = wah.columns.values_at_rows(wah, part, torch.arange(n, 32 * part[2], dtype=torch.int64, device="cuda"))
    assert not bool(behind[1].any()) and not bool(behind[0].any())


# ---- 8: graph capture ----------------------------------------------------------------------------------------------------------------
def test_graph_replay_with_other_pieces_and_sources(wah, oracle):
    """Pieces and table are only ever read by the device: ONE captured call, replayed after both were overwritten in place -- other
    first rows, other sources, the same counts -- splices the new pieces (capture as tests/test_gpu_bsi_build.py: side stream,
    warm-up outside, check=False; one chain of launches, no parallel branches)."""
    import torch

    n_out = 2 * SEG_WORDS

    def variant(seed, first):
        pieces = [(SEG_WORDS, first, 20000), (2 * SEG_WORDS, 3 * first + 1, 30000)]
        return sp.Case(f"replay {seed}", n_out, pieces, [sp._columns(SEG_WORDS, seed, sp.KINDS[:3]), sp._columns(2 * SEG_WORDS, seed + 9, sp.KINDS[1:])])

    variants = [variant(100, 0), variant(101, 77), variant(102, 3100), variant(103, 31)]
    all_ops = [Operands(oracle, v) for v in variants]
    pieces, table = all_ops[0].pieces.clone(), all_ops[0].table.clone()
    k = variants[0].n_columns
    sc = torch.empty(int(wah.lib().wah_splice_scratch_bytes(n_out, k, 2)), dtype=torch.uint8, device="cuda")
    res = torch.empty(k * wah.max_compressed_words(n_out), dtype=torch.int32, device="cuda")
    res_offs = torch.zeros(k * 2 + 1, dtype=torch.int64, device="cuda")
    wah.splice_device(pieces, table, k, n_out, scratch=sc, out=res, out_offsets=res_offs, check=False)  # warm-up outside the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _, count, _ = wah.splice_device(pieces, table, k, n_out, scratch=sc, out=res, out_offsets=res_offs, check=False)
    for i in (1, 2, 3, 0):
        pieces.copy_(all_ops[i].pieces)
        table.copy_(all_ops[i].table)
        res.fill_(GUARD)
        g.replay()
        torch.cuda.synchronize()
        assert wah.lib().wah_splice_status(sc.data_ptr(), None) == WAH_OK
        _check(variants[i], (res[: int(count.item())], res_offs), sp.reference(oracle, variants[i]))


# ---- 9: refusals ---------------------------------------------------------------------------------------------------------------------
def _status(wah, case, ops, pieces=None, table=None, cap=None):
    """The call with check=False and then its status: (code, out buffer, count, offsets)."""
    import torch

    k, n = case.n_columns, case.n_words_out
    pieces = ops.pieces if pieces is None else torch.tensor(pieces, dtype=torch.int64, device="cuda")
    table = ops.table if table is None else torch.tensor(table, dtype=torch.int64, device="cuda")
    sc = torch.empty(int(wah.lib().wah_splice_scratch_bytes(n, k, pieces.shape[0])), dtype=torch.uint8, device="cuda")
    full = k * wah.max_compressed_words(n)
    buf = torch.full((full + 1,), GUARD, dtype=torch.int32, device="cuda")
    out, count, offs = wah.splice_device(pieces, table, k, n, scratch=sc, out=buf[: full if cap is None else cap], check=False)
    code = wah.lib().wah_splice_status(sc.data_ptr(), None)
    return code, buf, int(count.item()), offs


def _two_pieces():
    return sp.Case("refusals", SEG_WORDS, [(SEG_WORDS, 100, 3000), (31, 1, 900)], [sp._columns(SEG_WORDS, 50, sp.KINDS[:2]), sp._columns(31, 53, sp.KINDS[:2])])


BAD_PIECES = {
    "rows of an operand of no words": [(SEG_WORDS, 100, 3000), (0, 0, 1)],
    "an operand of 2^40 words": [(SEG_WORDS, 100, 3000), (1 << 40, 1, 900)],
    "rows behind the operand": [(SEG_WORDS, 100, 3000), (31, 93, 900)],
    "first row behind the operand": [(SEG_WORDS, 100, 3000), (31, 993, 1)],
    "a sum that wraps": [(SEG_WORDS, 100, 3000), (31, 2, -1)],                      # n_rows = 2^64 - 1
    "a first row that wraps": [(SEG_WORDS, 100, 3000), (31, -1, 2)],
    "one piece of more rows than the output holds": [(2 * SEG_WORDS, 0, SEG_BITS + 1), (31, 1, 0)],
    "more rows than the output holds in all": [(SEG_WORDS, 0, SEG_BITS - 899), (31, 1, 900)],
}


@pytest.mark.parametrize("what", list(BAD_PIECES))
def test_a_bad_piece_is_a_stream_error(wah, oracle, what):
    case = _two_pieces()
    ops = Operands(oracle, case)
    assert _status(wah, case, ops)[0] == WAH_OK
    assert _status(wah, case, ops, pieces=BAD_PIECES[what])[0] == WAH_ERR_STREAM, what


def test_the_most_rows_the_output_holds_are_accepted(wah, oracle):
    case = sp.Case("exactly full", SEG_WORDS, [(SEG_WORDS, 0, SEG_BITS - 900), (31, 1, 900)], _two_pieces().sources)
    _check(case, _run(wah, case, Operands(oracle, case)), sp.reference(oracle, case))


@pytest.mark.parametrize("what", ("null stream", "null index", "misaligned stream", "misaligned index", "index range outside the stream"))
def test_a_bad_operand_of_a_piece_with_rows_is_a_stream_error(wah, oracle, what):
    case = _two_pieces()
    ops = Operands(oracle, case)
    table = [list(r) for r in ops.host_table()]
    row = table[3]  # (piece 1, column 1)
    if what == "null stream":
        row[0] = 0
    elif what == "null index":
        row[2] = 0
    elif what == "misaligned stream":
        row[0] += 2
    elif what == "misaligned index":
        row[2] += 4
    else:
        row[1] = 1  # the stream is said to be one word long: the segment's range ends behind it
        assert ops.rows[3][1] > 1
    assert _status(wah, case, ops, table=table)[0] == WAH_ERR_STREAM, what
    # the same entry under a piece of no rows is never followed
    code, buf, count, offs = _status(wah, case, ops, pieces=[case.pieces[0], (31, 1, 0)], table=table)
    assert code == WAH_OK
    want = sp.reference(oracle, sp.Case("one piece", SEG_WORDS, [case.pieces[0], (31, 1, 0)], case.sources))
    assert count == want[0].size and np.array_equal(_host(buf[:count]), want[0]) and np.array_equal(offs.cpu().numpy(), want[1])


def test_a_malformed_segment_is_refused_only_where_it_is_read(wah, oracle):
    n = 2 * SEG_WORDS
    src = sp.source("clustered", n, 110)
    st = np.ascontiguousarray(oracle.compress(src), dtype=np.uint32)
    idx = _select.index_of(st)
    fills = np.flatnonzero(st[idx[1]:] & np.uint32(sp.FILL0)) + idx[1]
    bad = st.copy()
    bad[fills[fills.size // 2]] += 1  # a fill of segment 1 one group too long: the segment's words no longer make up its groups
    reads = sp.Case("reads segment 1", SEG_WORDS, [(n, SEG_BITS - 5, 1000)], [[src]])
    stays = sp.Case("stays in segment 0", SEG_WORDS, [(n, 5, SEG_BITS - 5)], [[src]])
    assert _status(wah, reads, Operands(oracle, reads, {(0, 0): (bad, idx)}))[0] == WAH_ERR_STREAM
    _check(stays, _run(wah, stays, Operands(oracle, stays, {(0, 0): (bad, idx)})), sp.reference(oracle, stays))
    _check(reads, _run(wah, reads, Operands(oracle, reads)), sp.reference(oracle, reads))


def test_capacity(wah, oracle):
    case = _two_pieces()
    ops = Operands(oracle, case)
    want = sp.reference(oracle, case)
    total = want[0].size
    code, buf, count, offs = _status(wah, case, ops, cap=total)
    assert code == WAH_OK and count == total and np.array_equal(_host(buf[:total]), want[0]) and int(buf[total].item()) == GUARD
    code, buf, count, offs = _status(wah, case, ops, cap=total - 1)
    assert code == WAH_ERR_CAPACITY and count == total
    assert bool((buf[total - 1:] == GUARD).all()), "a word at or behind the capacity was written"
    assert np.array_equal(_host(buf[: total - 1]), want[0][: total - 1])

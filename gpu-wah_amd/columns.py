"""Column sharding for many independent bitmaps (BASELINE.json configs[4]).

Bitmap columns are unrelated, so a node with N GPUs is N independent compressors: column c belongs to rank
c mod N, every rank walks its own columns on its own device and streams, and the only cross-rank step is
adding up byte counts and taking the slowest rank's time.  No collective touches bitmap data.

The reference has no multi-device code at all (single device, default stream: compress.cu:129,166); this
module is the "many columns" driver a caller of the reference would have written around compress().
"""
from collections import namedtuple

ColumnSpec = namedtuple("ColumnSpec", "index kind seed n_words")

KINDS = ("sparse", "clustered", "dense")  # uniform p=0.01 / runs of mean 4096 bits / uniform p=0.5


def shard_columns(n_columns, rank, world):
    """Indices of the columns rank `rank` of `world` owns: c with c % world == rank (round robin)."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    return list(range(rank, n_columns, world))


def column_spec(index, n_words, seed=1337):
    """Deterministic description of synthetic column `index`: the three bench distributions in turn."""
    return ColumnSpec(index, KINDS[index % len(KINDS)], seed + index, n_words)


def make_column(wah, spec, device, out=None):
    """Generate the column in HBM on `device` (bit-exact definition: include/wah_gen.h); `out`: into this tensor."""
    if spec.kind == "sparse":
        return wah.gen_uniform_device(spec.n_words, spec.seed, 0.01, device=device, out=out)
    if spec.kind == "dense":
        return wah.gen_uniform_device(spec.n_words, spec.seed, 0.5, device=device, out=out)
    return wah.gen_clustered_device(spec.n_words, spec.seed, 4096, device=device, out=out)


SEGMENT_WORDS = 992  # one reference block: fills never cross it


def make_column_matrix(wah, specs, device):
    """The columns of `specs` (equal lengths, whole 992-word segments) as ONE tensor [len(specs), n_words]."""
    import torch

    n = specs[0].n_words
    if any(sp.n_words != n for sp in specs) or n % SEGMENT_WORDS:
        raise ValueError("a column matrix needs equal column lengths that are multiples of 992 words")
    m = torch.empty((len(specs), n), dtype=torch.int32, device=device)
    for row, sp in zip(m, specs):
        make_column(wah, sp, device, out=row)
    return m


def compress_column_matrix(compressor, matrix, wait=True):
    """All columns of a contiguous [columns, n_words] matrix in ONE launch (n_words a multiple of 992).

    Fills are maximal inside a 992-word segment and never cross one (F4), and every column is a whole number of
    segments, so compressing the matrix as one long bitmap yields exactly the columns' streams back to back; the
    segment index of the `indexed` compressor says where each one starts.  Returns (stream, column_offsets): column c
    is stream[column_offsets[c] : column_offsets[c + 1]], bit-identical to compressing it alone.  wait=False: only
    enqueue the launch (read compressor.result() / .seg_offsets after synchronising)."""
    columns, n = matrix.shape
    if n % SEGMENT_WORDS or not matrix.is_contiguous():
        raise ValueError("columns must be contiguous and a multiple of 992 words long")
    if compressor.seg_offsets is None:
        raise ValueError("needs DeviceCompressor(..., indexed=True)")
    compressor.run(matrix.view(-1))
    if not wait:
        return None, None
    stream = compressor.result()
    segs = n // SEGMENT_WORDS
    return stream, compressor.seg_offsets[:: segs][: columns + 1]


def column_operand_table(stream, seg_offsets, n_words_per_column, column_ids, out=None):
    """The operand table (include/wah.h: wah_bitop_operand; api.bitop_operand_table) that selects columns of a
    compress_column_matrix result by their numbers, built ON THE DEVICE: `stream` is the whole matrix stream, `seg_offsets`
    the compressor's whole index (DeviceCompressor.seg_offsets, not the per-column slice), and column c is the window
    whose index starts at entry c * n_words_per_column / 992.  column_ids: an int64 device tensor (no host round trip: the
    numbers are not checked against the matrix, the caller vouches for them) or a Python list.  out: an existing
    [len(column_ids), 3] table to overwrite in place -- what a captured graph replayed with another selection needs.
    Like every table it holds raw pointers: keep `stream` and `seg_offsets` alive."""
    import torch

    if n_words_per_column % SEGMENT_WORDS or n_words_per_column <= 0:
        raise ValueError("columns of a column matrix are a multiple of 992 words long")
    segs = n_words_per_column // SEGMENT_WORDS
    if not torch.is_tensor(column_ids):
        ids = [int(c) for c in column_ids]
        if not ids or min(ids) < 0 or (max(ids) + 1) * segs + 1 > seg_offsets.numel():
            raise ValueError("column numbers outside the matrix")
        column_ids = torch.tensor(ids, dtype=torch.int64, device=stream.device)
    if column_ids.dtype != torch.int64 or column_ids.dim() != 1 or column_ids.numel() < 1 or column_ids.device != stream.device:
        raise ValueError("column_ids: a non-empty one-dimensional int64 tensor on the stream's device")
    if seg_offsets.dtype != torch.int64 or not seg_offsets.is_contiguous() or seg_offsets.device != stream.device:
        raise ValueError("seg_offsets: the compressor's contiguous int64 index")
    if out is None:
        out = torch.empty((column_ids.numel(), 3), dtype=torch.int64, device=stream.device)
    elif out.dtype != torch.int64 or tuple(out.shape) != (column_ids.numel(), 3) or not out.is_contiguous() or out.device != stream.device:
        raise ValueError("out: a contiguous int64 [len(column_ids), 3] tensor on the stream's device")
    out[:, 0] = stream.data_ptr()
    out[:, 1] = stream.numel()
    out[:, 2] = column_ids * (segs * 8) + seg_offsets.data_ptr()
    return out


def combine_columns(wah, op, stream, seg_offsets, n_words_per_column, column_ids, **reuse):
    """`value IN (...)` / `lo <= value <= hi` on an equality-encoded index in one call: op ("or", "and", "xor", "andnot") over
    the selected columns of a compress_column_matrix result, any number of them (wah_bitop_list_indexed_device).  Arguments
    as column_operand_table; reuse: scratch / out / out_offsets / check of api.bitop_list_indexed_device.  Returns
    (stream, seg_offsets) of the result bitmap."""
    table = column_operand_table(stream, seg_offsets, n_words_per_column, column_ids)
    return wah.bitop_list_indexed_device(op, table, n_words_per_column, **reuse)


def filter_columns(wah, predicates, n_words_per_column, tables=None, **reuse):
    """A conjunction of predicates over SEVERAL attributes in one call (wah_bitop_clauses_indexed_device): predicates is a
    list of (stream, seg_offsets, column_ids, negate), one per attribute, each naming columns of its OWN
    compress_column_matrix result (arguments as column_operand_table; all matrices of one column length).  A predicate is
    `attribute IN (its columns)`, negate: NOT IN; the result is their AND.  tables: an existing (operand_table, clause_ends)
    pair of the same counts to overwrite in place -- what a captured graph replayed with another query needs; reuse:
    scratch / out / out_offsets / check of api.bitop_clauses_indexed_device.  Device-resident column_ids cause no host
    round trip.  Returns (stream, seg_offsets) of the result bitmap."""
    import torch

    if not predicates:
        raise ValueError("at least one predicate")
    sizes = [int(ids.numel()) if torch.is_tensor(ids) else len(ids) for _, _, ids, _ in predicates]
    if min(sizes) < 1:
        raise ValueError("a predicate names at least one column")
    dev = predicates[0][0].device
    ends, total = [], 0
    for size, (_, _, _, negate) in zip(sizes, predicates):
        total += size
        ends.append(total | (wah.CLAUSE_NEGATE if negate else 0))
    if tables is None:
        table = torch.empty((total, 3), dtype=torch.int64, device=dev)
        clause_ends = torch.empty(len(ends), dtype=torch.int64, device=dev)
    else:
        table, clause_ends = tables
        if tuple(table.shape) != (total, 3) or tuple(clause_ends.shape) != (len(ends),) or clause_ends.dtype != torch.int64:
            raise ValueError("tables: an int64 [operands, 3] table and an int64 [predicates] tensor of this query's counts")
    clause_ends.copy_(torch.tensor(ends, dtype=torch.int64))
    at = 0
    for size, (stream, seg_offsets, ids, _) in zip(sizes, predicates):
        column_operand_table(stream, seg_offsets, n_words_per_column, ids, out=table[at: at + size])
        at += size
    return wah.bitop_clauses_indexed_device((table, clause_ends), n_words_per_column, **reuse)


def count_columns(wah, stream, seg_offsets, n_words_per_column, column_ids, **reuse):
    """The set bits of each selected column of a compress_column_matrix result, in one call (wah_count_list_indexed_device):
    over all columns of an equality-encoded attribute the `GROUP BY value` histogram.  Arguments as column_operand_table;
    reuse: scratch / counts / check of api.count_device.  Device-resident column_ids cause no host round trip.  Returns an
    int64 tensor [len(column_ids)]."""
    table = column_operand_table(stream, seg_offsets, n_words_per_column, column_ids)
    return wah.count_device(table, n_words_per_column, **reuse)


def count_columns_where(wah, predicates, stream, seg_offsets, n_words_per_column, column_ids, **reuse):
    """`SELECT b, COUNT(*) WHERE <conjunction> GROUP BY b` in two calls that decode no bitmap: filter_columns (predicates as
    there), then the set bits each selected column of attribute b's matrix (stream, seg_offsets, column_ids as
    column_operand_table) shares with its result (wah_count_masked_indexed_device).  With device-resident column_ids there is no
    host round trip between the two: the filter is only enqueued, the mask row names its output buffer with the buffer's
    capacity as the length -- the index it wrote bounds what is read -- and one check comes at the end.  reuse: scratch / counts
    ([1, len(column_ids)]) / check of api.count_masked_device, and filter=dict(...) with tables / scratch / out / out_offsets
    of filter_columns (check=False reads no status at all: pass the filter's scratch to read its own later).  Returns an int64
    tensor [len(column_ids)]."""
    import torch

    filter_reuse = dict(reuse.pop("filter", None) or {})
    check = reuse.pop("check", True)
    n = int(n_words_per_column)
    table = column_operand_table(stream, seg_offsets, n, column_ids)
    dev = table.device
    if filter_reuse.get("scratch") is None:
        total = sum(int(ids.numel()) if torch.is_tensor(ids) else len(ids) for _, _, ids, _ in predicates)
        filter_reuse["scratch"] = torch.empty(int(wah.lib().wah_bitop_clauses_scratch_bytes(n, total, len(predicates))), dtype=torch.uint8, device=dev)
    filter_reuse["check"] = False
    out, _, out_offsets = filter_columns(wah, predicates, n, **filter_reuse)
    mask = torch.empty((1, 3), dtype=torch.int64, device=dev)
    mask[0, 0] = out.data_ptr()
    mask[0, 1] = out.numel()
    mask[0, 2] = out_offsets.data_ptr()
    scratch = reuse.pop("scratch", None)
    if scratch is None:
        scratch = torch.empty(int(wah.lib().wah_select_scratch_bytes(n, table.shape[0])), dtype=torch.uint8, device=dev)
    counts = wah.count_masked_device(mask, table, n, scratch=scratch, check=False, **reuse)
    if check:
        from . import api

        sp = api._stream_ptr(torch)
        api._check(wah.lib().wah_bitop_clauses_status(filter_reuse["scratch"].data_ptr(), n, 1, 1, sp), "count_columns_where: the filter")
        api._check(wah.lib().wah_select_status(scratch.data_ptr(), sp), "count_columns_where: the count")
    return counts.view(-1)


def crosstab_columns(wah, a, b, n_words_per_column, **reuse):
    """`SELECT a, b, COUNT(*) GROUP BY a, b` over two equality-encoded attributes in one call (wah_count_masked_indexed_device):
    a and b are each (stream, seg_offsets, column_ids) of a compress_column_matrix result of its own (arguments as
    column_operand_table; one column length); the columns of a are the masks, those of b the operands.  reuse: scratch / counts
    / check of api.count_masked_device.  Returns an int64 tensor [len(a's column_ids), len(b's column_ids)]."""
    masks = column_operand_table(a[0], a[1], n_words_per_column, a[2])
    operands = column_operand_table(b[0], b[1], n_words_per_column, b[2])
    return wah.count_masked_device(masks, operands, n_words_per_column, **reuse)


def select_rows(wah, predicates, n_words_per_column, first=0, limit=None):
    """`SELECT rowid ... WHERE <conjunction> LIMIT limit OFFSET first` in two calls that never decode a bitmap: filter_columns
    (predicates as there), then api.positions_device over its result.  Returns (row numbers int64 tensor, matching rows)."""
    result, result_offsets = filter_columns(wah, predicates, n_words_per_column)
    return wah.positions_device(result, result_offsets, n_words_per_column, first=first, limit=limit)


def bitmaps_from_rows(wah, row_lists, n_words, **reuse):
    """One compressed bitmap of n_words words per list of row numbers, in one call and without a decoded bitmap
    (wah_from_positions_device): row_lists is a Python list of int64 device tensors, each strictly ascending (a join's row ids, a
    tombstone list; an empty tensor is an empty bitmap).  reuse: scratch / out / out_offsets / check of
    api.from_positions_device.  Returns its (stream, seg_offsets): list c is the operand (stream, seg_offsets[c * S:]), S the
    segments of one bitmap; with n_words a multiple of 992 the pair goes into column_operand_table as a column matrix does."""
    import torch

    if not row_lists:
        raise ValueError("at least one list")
    dev = row_lists[0].device
    rows = torch.cat([r.reshape(-1) for r in row_lists]).contiguous()
    ends = torch.tensor([int(r.numel()) for r in row_lists], dtype=torch.int64).cumsum(0).to(dev)
    return wah.from_positions_device(rows, ends, n_words, **reuse)


def index_from_keys(wah, keys, n_values, n_words_per_column=None, check=True):
    """The equality-encoded bitmap index of a key column without its decoded bit matrix [n_values, rows / 32]: keys is an int64
    device tensor with one value in [0, n_values) per row.  Grouping the rows is plumbing -- one stable torch.sort, whose indices
    are each value's rows in ascending order, and one torch.bincount, whose running sum is where each value's rows end --; the
    bitmaps are one wah_from_positions_device call.  n_words_per_column defaults to ceil(rows / 32) rounded up to a multiple of
    992.  check=True: keys outside [0, n_values) raise (one host read of their minimum and maximum) and the call's status is read;
    check=False reads nothing back and returns the whole output buffer.  Returns (stream, seg_offsets, n_words_per_column), which
    go in as the arguments of the same names of column_operand_table, combine_columns, filter_columns, count_columns,
    crosstab_columns and select_rows."""
    import torch

    if keys.dtype != torch.int64 or keys.dim() != 1 or not keys.is_cuda:
        raise ValueError("keys: a one-dimensional int64 device tensor")
    n_values, rows = int(n_values), int(keys.numel())
    if n_values < 1:
        raise ValueError("at least one value")
    if n_words_per_column is None:
        n_words_per_column = max(-(-((rows + 31) // 32) // SEGMENT_WORDS), 1) * SEGMENT_WORDS
    n = int(n_words_per_column)
    if n % SEGMENT_WORDS or n <= 0 or 32 * n < rows:
        raise ValueError("columns are a multiple of 992 words long and hold every row")
    if check and rows:
        lo, hi = (int(v) for v in torch.aminmax(keys))
        if lo < 0 or hi >= n_values:
            raise ValueError(f"keys outside [0, {n_values})")
    order = torch.sort(keys, stable=True).indices
    ends = torch.bincount(keys, minlength=n_values)[:n_values].cumsum(0)
    if not check:
        out, _, out_offsets = wah.from_positions_device(order, ends, n, check=False)
        return out, out_offsets, n
    stream, seg_offsets = wah.from_positions_device(order, ends, n)
    return stream, seg_offsets, n


def _bsi_arguments(values, n_bits, n_words_per_column, exists):
    """What bsi_from_values asks of its arguments; returns (n_bits, rows, n_words_per_column) as Python ints."""
    import torch

    if values.dtype != torch.int64 or values.dim() != 1 or not values.is_cuda:
        raise ValueError("values: a one-dimensional int64 device tensor")
    n_bits, rows = int(n_bits), int(values.numel())
    if not 1 <= n_bits <= 63:
        raise ValueError("between 1 and 63 bits")
    if exists is not None and (exists.dtype != torch.bool or tuple(exists.shape) != (rows,) or exists.device != values.device):
        raise ValueError("exists: a bool tensor of the values' length on their device")
    if n_words_per_column is None:
        n_words_per_column = max(-(-((rows + 31) // 32) // SEGMENT_WORDS), 1) * SEGMENT_WORDS
    n = int(n_words_per_column)
    if n % SEGMENT_WORDS or n <= 0 or 32 * n < rows:
        raise ValueError("columns are a multiple of 992 words long and hold every row")
    return n_bits, rows, n


def bsi_from_values(wah, values, n_bits, n_words_per_column=None, exists=None, check=True):
    """The bit-sliced index of a value column (O'Neil & Quass): one bitmap per BIT of the value instead of one per distinct
    value, what a price, a timestamp or an id needs.  values: an int64 device tensor with one value in [0, 2^n_bits) per row,
    n_bits <= 63; exists: a bool device tensor of the same length, the rows that have a value at all (their values elsewhere
    are stored as 0), or None.  One call (api.bsi_build_device, wah_bsi_build_device): the column is transposed on the device
    into the decoded slice matrix [n_bits (+ 1), n_words], MOST significant slice first and the existence row last, and that is
    compressed in one launch -- slices are mostly incompressible, which is the compressor's own road.  n_words_per_column
    defaults to ceil(rows / 32) rounded up to a multiple of 992.  check=True: values outside [0, 2^n_bits) raise ValueError (the
    call's status is read: no value is read back); check=False reads nothing back and returns the whole output buffer.  Returns
    (stream, seg_offsets, n_words_per_column, n_bits, has_exists): the first three go into column_operand_table as a column
    matrix's do (slice i is column i, the existence bitmap column n_bits), the tuple as a whole into range_column,
    compare_column, compare_columns and sum_column_where."""
    import torch

    from . import api

    n_bits, rows, n = _bsi_arguments(values, n_bits, n_words_per_column, exists)
    has_exists = exists is not None
    n_slices = n_bits + (1 if has_exists else 0)
    values = values.contiguous()
    if has_exists:
        exists = exists.contiguous()
    scratch = torch.empty(int(wah.lib().wah_bsi_build_scratch_bytes(n, n_slices)), dtype=torch.uint8, device=values.device)
    out, count, out_offsets = wah.bsi_build_device(values, n_bits, n, exists=exists, scratch=scratch, check=False)
    if not check:
        return out, out_offsets, n, n_bits, has_exists
    rc = int(wah.lib().wah_bsi_build_status(scratch.data_ptr(), n, n_slices, api._stream_ptr(torch)))
    if rc == -6:  # WAH_ERR_STREAM: the transpose saw a value at or above 2^n_bits (a negative one is 2^63 or more)
        raise ValueError(f"values outside [0, 2^{n_bits})")
    api._check(rc, "bsi_from_values")
    return out[: int(count.item())], out_offsets, n, n_bits, has_exists


def _bsi_from_values_torch(wah, values, n_bits, n_words_per_column=None, exists=None):
    """bsi_from_values as it was before wah_bsi_build_device, kept to be compared against (tools/bsi_build_time.py, the tests): the
    decoded slice matrix is made with torch ops, one slice after the other, and compressed in one launch (compress_column_matrix);
    the values' minimum and maximum are read back to the host.  Arguments and result as bsi_from_values with check=True."""
    import torch

    n_bits, rows, n = _bsi_arguments(values, n_bits, n_words_per_column, exists)
    if rows:
        lo, hi = (int(v) for v in torch.aminmax(values))
        if lo < 0 or hi >= 1 << n_bits:
            raise ValueError(f"values outside [0, 2^{n_bits})")
    dev = values.device
    weights = torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, dtype=torch.int64, device=dev)

    def pack(bits, row):  # bits: int64 0 / 1 per row -> the bitmap's words, position 32 * word + bit
        padded = torch.zeros(32 * n, dtype=torch.int64, device=dev)
        padded[:rows] = bits
        words = (padded.view(n, 32) * weights).sum(1)
        row.copy_(torch.where(words >= 1 << 31, words - (1 << 32), words))

    have = None if exists is None else exists.to(torch.int64)
    matrix = torch.empty((n_bits + (exists is not None), n), dtype=torch.int32, device=dev)
    for i in range(n_bits):
        bits = (values >> (n_bits - 1 - i)) & 1
        pack(bits if have is None else bits & have, matrix[i])
    if have is not None:
        pack(have, matrix[n_bits])
    comp = wah.DeviceCompressor(matrix.numel(), device=dev, indexed=True)
    stream, _ = compress_column_matrix(comp, matrix)
    return stream, comp.seg_offsets, n, n_bits, exists is not None


def range_column(wah, bsi, lo, hi, table=None, bounds=None, **reuse):
    """`lo <= value <= hi` (both inclusive) over a bit-sliced attribute in one call (wah_bsi_range_indexed_device): bsi is what
    bsi_from_values returned, lo and hi Python ints up to 2^64 - 1 -- an empty range is all zeros, hi beyond the attribute's
    width its maximum.  table / bounds: an existing [n_bits (+ 1), 3] slice table and int64 [2] bounds tensor to overwrite in
    place -- what a captured graph replayed with another range needs; reuse: scratch / out / out_offsets / check of
    api.bsi_range_device.  Returns (stream, seg_offsets) of the result bitmap, usable as a predicate's single column in
    filter_columns: (stream, seg_offsets, [0], negate) with the result's own length as the column length."""
    stream, seg_offsets, n, n_bits, has_exists = bsi
    table = column_operand_table(stream, seg_offsets, n, list(range(n_bits + (1 if has_exists else 0))), out=table)
    bounds = wah.bsi_bounds(lo, hi, stream.device, out=bounds)
    return wah.bsi_range_device(table, bounds, n, exists=has_exists, **reuse)


def _sort_unsigned(values):
    """An int64 tensor of 64-bit patterns in non-decreasing UNSIGNED order (the order wah_bsi_member_indexed_device wants): the
    sign bit is flipped around a signed torch.sort."""
    import torch

    top = -(1 << 63)
    return (torch.sort(values.reshape(-1) ^ top)[0] ^ top).contiguous()


def _slice_table(bsi):
    """The slice table of a bit-sliced attribute in sweep order: its slices, most significant first, then its existence bitmap."""
    stream, seg_offsets, n, n_bits, has_exists = bsi
    return column_operand_table(stream, seg_offsets, n, list(range(n_bits + (1 if has_exists else 0))))


def isin_column(wah, bsi, values, negate=False, **reuse):
    """`value IN (values)`, with negate=True `value NOT IN (values)`, over a bit-sliced attribute in one call
    (wah_bsi_member_indexed_device): bsi is what bsi_from_values returned; values: Python ints up to 2^64 - 1 or a numpy uint64
    array (api.member_set), or an int64 DEVICE tensor of 64-bit patterns in any order, which is sorted on the device -- nothing
    of it is read back.  Duplicates are allowed, an empty list is an empty set, a value beyond the attribute's width matches
    nothing.  Rows without a value (the existence bitmap) are in neither result.  reuse: count / scratch / out / out_offsets /
    check of api.bsi_member_device.  Returns (stream, seg_offsets) of the result bitmap, a predicate like range_column's."""
    import torch

    stream, _, n, _, has_exists = bsi
    members = _sort_unsigned(values) if torch.is_tensor(values) else wah.member_set(values, stream.device)
    return wah.bsi_member_device(_slice_table(bsi), members, n, exists=has_exists, negate=negate, **reuse)


def semi_join_rows(wah, bsi_fk, dim_mask, dim_n_words, negate=False, **reuse):
    """The star join's probe: the fact rows whose foreign key -- a ROW NUMBER of the dimension table, the bit-sliced attribute
    bsi_fk -- is a row that dim_mask selects (`WHERE fk IN (SELECT rowid FROM dim WHERE ...)`), in one call
    (wah_bsi_member_indexed_device, WAH_MEMBER_BITSET).  dim_mask: (stream, seg_offsets) of an indexed compressed bitmap of
    dim_n_words words, a filter_columns or range_column result over the dimension table.  It is decoded once
    (api.decompress_segments_device) and its words ARE the set, 32 * dim_n_words bits: a key at or beyond them matches nothing.
    negate: the rows whose key is not selected; rows without a key are in neither result.  reuse: scratch / out / out_offsets /
    check of api.bsi_member_device.  Returns (stream, seg_offsets) of the result bitmap."""
    stream, _, n, _, has_exists = bsi_fk
    m = int(dim_n_words)
    words = wah.decompress_segments_device(dim_mask[0], dim_mask[1], m)[:m].contiguous()
    return wah.bsi_member_device(_slice_table(bsi_fk), words, n, exists=has_exists, negate=negate, bitset=True, set_bits=32 * m, **reuse)


def semi_join_values(wah, bsi, bsi_other, other_mask=None, negate=False, other_rows=None, capacity=None, **reuse):
    """The rows of one attribute whose value occurs in another (`a.x IN (SELECT y FROM b WHERE ...)`): the other attribute's
    values become a sorted list on the device and one wah_bsi_member_indexed_device call probes it.  bsi, bsi_other: what
    bsi_from_values returned, of any two lengths and widths.  Rows of bsi_other without a value (its existence bitmap) do not
    enter the set; WITHOUT an existence bitmap every row of its bitmaps has a value, the rows behind the caller's own count the
    value 0 -- other_rows cuts the set to the first other_rows rows.
      other_mask=None  the set is values_of_column(bsi_other), a torch.sort follows, and the count (the rows that have a
                       value) stays in a device tensor: nothing is read back;
      other_mask       (stream, seg_offsets), a bitmap over bsi_other's rows: the set is values_at_rows of select_rows.  The
                       number of selected rows is READ BACK ONCE to size the list -- unless capacity= is given: the list then
                       has that many entries, padded with UINT64_MAX behind the selected rows' values, and the count stays on the
                       device; more selected rows than capacity are refused by the call's status (a count above the capacity).
    negate: the rows whose value does not occur; rows of bsi without a value are in neither result.  reuse: scratch / out /
    out_offsets / check of api.bsi_member_device.  Returns (stream, seg_offsets) of the result bitmap."""
    import torch

    stream, _, n, _, has_exists = bsi
    o_stream, o_offsets, o_n, o_bits, o_exists = bsi_other
    count = None
    if other_mask is None:
        if capacity is not None:
            raise ValueError("capacity sizes the list of a masked set")
        values, have = values_of_column(wah, bsi_other, 0, other_rows)
        if have is not None:
            values = torch.where(have, values, torch.full_like(values, -1))  # (UINT64_MAX: sorted behind every counted entry)
            count = have.sum().reshape(1)
    else:
        if other_rows is not None:
            raise ValueError("other_rows cuts an unmasked set: a mask selects its own rows")
        predicates = [(other_mask[0], other_mask[1], [0], False)]
        if o_exists:
            predicates.append((o_stream, o_offsets, [o_bits], False))
        if capacity is None:
            rows, _ = select_rows(wah, predicates, o_n)
            values, _ = values_at_rows(wah, bsi_other, rows)
        else:
            selected, selected_offsets = filter_columns(wah, predicates, o_n)
            rows = torch.zeros(int(capacity), dtype=torch.int64, device=stream.device)
            rows, info = wah.positions_device(selected, selected_offsets, o_n, limit=int(capacity), out=rows, check=False)
            values, _ = values_at_rows(wah, bsi_other, rows)
            count = info[:1].contiguous()  # (the total: above the capacity the call refuses it)
            values = torch.where(torch.arange(int(capacity), device=stream.device) < count, values, torch.full_like(values, -1))
    return wah.bsi_member_device(_slice_table(bsi), _sort_unsigned(values), n, count=count, exists=has_exists, negate=negate, **reuse)


def compare_column(wah, bsi, op, c, **reuse):
    """`value op c` over a bit-sliced attribute, op one of "<", "<=", ">", ">=", "==", as the matching range of range_column
    ("<" with c == 0 and ">" with c at the attribute's maximum are empty ranges, not errors; != is == as a negated predicate of
    filter_columns).  Arguments and result as range_column."""
    n_bits = bsi[3]
    top, c = (1 << n_bits) - 1, int(c)
    if c < 0:
        raise ValueError("values are unsigned")
    empty = (1, 0)
    if op == "<":
        lo, hi = (0, c - 1) if c > 0 else empty
    elif op == "<=":
        lo, hi = 0, c
    elif op == ">":
        lo, hi = (c + 1, top) if c < top else empty
    elif op == ">=":
        lo, hi = (c, top) if c <= top else empty
    elif op == "==":
        lo, hi = (c, c) if c <= top else empty
    else:
        raise ValueError('op: one of "<", "<=", ">", ">=", "=="')
    return range_column(wah, bsi, lo, min(hi, (1 << 64) - 1), **reuse)


def compare_columns(wah, bsi_a, op, bsi_b, table=None, **reuse):
    """`A op B` row by row over TWO bit-sliced attributes in one call (wah_bsi_compare_indexed_device): bsi_a and bsi_b are what
    bsi_from_values returned for two value columns of the same column length, their widths may differ; op one of "<", "<=", ">",
    ">=", "==", "!=", both values read as unsigned.  The result is ANDed with every existence bitmap there is; without one the
    rows behind the caller's own hold 0 in both attributes and match "==", "<=" and ">=".  The table interleaves the two
    attributes' slices by significance (api.bsi_compare_row_order), each attribute's rows from column_operand_table.  table: an
    existing [rows, 3] table to overwrite in place -- what a captured graph replayed over other attributes of the same widths
    needs; reuse: scratch / out / out_offsets / check of api.bsi_compare_device.  Returns (stream, seg_offsets) of the result
    bitmap, usable as a predicate in filter_columns like a range_column result."""
    if op not in wah.CMP_OPS:
        raise ValueError('op: one of "<", "<=", ">", ">=", "==", "!="')
    _, _, n, ka, has_a = bsi_a
    _, _, n_b, kb, has_b = bsi_b
    if n != n_b:
        raise ValueError("the two attributes have different column lengths")
    table = _two_attribute_table(wah.bsi_compare_row_order(ka, kb, has_a, has_b), bsi_a, bsi_b, table)
    return wah.bsi_compare_device(table, ka, kb, op, n, exists_a=has_a, exists_b=has_b, **reuse)


def _two_attribute_table(order, bsi_a, bsi_b, table=None):
    """The row table of a call over TWO bit-sliced attributes of one column length: order is the call's table order, a list of
    (attribute "a" or "b", column of that attribute) as api.bsi_compare_row_order and api.bsi_arith_row_order state it; each
    attribute's rows come from column_operand_table.  table: an existing [rows, 3] table to overwrite in place."""
    import torch

    n, dev = bsi_a[2], bsi_a[0].device
    if table is None:
        table = torch.empty((len(order), 3), dtype=torch.int64, device=dev)
    elif table.dtype != torch.int64 or tuple(table.shape) != (len(order), 3) or not table.is_contiguous() or table.device != dev:
        raise ValueError("table: a contiguous int64 [rows, 3] tensor on the streams' device, one row per slice and existence bitmap")
    for name, (stream, offsets, *_) in (("a", bsi_a), ("b", bsi_b)):
        rows = [j for j, (who, _) in enumerate(order) if who == name]
        part = column_operand_table(stream, offsets, n, [c for who, c in order if who == name])
        table.index_copy_(0, torch.tensor(rows, dtype=torch.int64, device=dev), part)
    return table


def _arith_columns(wah, op, bsi_a, bsi_b, n_bits, table, reuse):
    """add_columns / subtract_columns: one wah_bsi_arith_indexed_device call over two bsi_from_values results."""
    import torch

    from . import api

    _, _, n, ka, has_a = bsi_a
    _, _, n_b, kb, has_b = bsi_b
    if n != n_b:
        raise ValueError("the two attributes have different column lengths")
    n_bits = min(max(ka, kb) + 1, 63) if n_bits is None else int(n_bits)
    if not 1 <= n_bits <= 64:
        raise ValueError("between 1 and 64 bits")
    table = _two_attribute_table(wah.bsi_arith_row_order(ka, kb, has_a, has_b), bsi_a, bsi_b, table)
    has_exists = bool(has_a or has_b)
    flags = (wah.BSI_EXISTS_A if has_a else 0) | (wah.BSI_EXISTS_B if has_b else 0)
    check = reuse.pop("check", True)
    if reuse.get("scratch") is None:
        reuse["scratch"] = torch.empty(int(wah.lib().wah_bsi_arith_scratch_bytes(n, n_bits, flags)), dtype=torch.uint8, device=table.device)
    out, count, out_offsets = wah.bsi_arith_device(table, ka, kb, op, n_bits, n, exists_a=has_a, exists_b=has_b, check=False, **reuse)
    if not check:
        return out, out_offsets, n, n_bits, has_exists
    api._check(wah.lib().wah_bsi_arith_status(reuse["scratch"].data_ptr(), n, n_bits, flags, api._stream_ptr(torch)), "bsi_arith")
    return out[: int(count.item())], out_offsets, n, n_bits, has_exists


def add_columns(wah, bsi_a, bsi_b, n_bits=None, table=None, **reuse):
    """`A + B` row by row over TWO bit-sliced attributes in one call, as a NEW bit-sliced attribute (wah_bsi_arith_indexed_device):
    bsi_a and bsi_b are what bsi_from_values -- or an earlier add_columns / subtract_columns -- returned for two value columns of
    the same column length, their widths may differ, both values read as unsigned.  The result holds (A + B) mod 2^n_bits;
    n_bits defaults to min(max(ka, kb) + 1, 63), which loses no carry below 63 bits (63 is the width this module handles
    elsewhere; the call itself takes 1 .. 64).  With an existence bitmap in either attribute the result has one, the AND of those
    present, and a row outside it is stored as 0.  The table puts the existence rows first and interleaves the slices least
    significant first (api.bsi_arith_row_order).  table: an existing [rows, 3] table to overwrite in place -- what a captured
    graph replayed over other attributes of the same widths needs; reuse: scratch / out / out_offsets / check of
    api.bsi_arith_device.  Returns the five-tuple of bsi_from_values (stream, seg_offsets, n_words_per_column, n_bits,
    has_exists), which goes into range_column, compare_columns, sum_column_where, kth_column_where, values_at_rows and another
    add_columns as it is; check=False reads nothing back and returns the whole output buffer, as there."""
    return _arith_columns(wah, "+", bsi_a, bsi_b, n_bits, table, reuse)


def subtract_columns(wah, bsi_a, bsi_b, n_bits=None, table=None, **reuse):
    """`A - B` row by row, arguments and result as add_columns.  The result holds (A - B) mod 2^n_bits, the two's-complement
    difference: with the default n_bits = max(ka, kb) + 1 the MOST significant slice (column 0 of the result) is the borrow, set
    exactly in the rows where A < B: the value is A - B where A >= B and 2^n_bits - (B - A) where not; a larger n_bits extends
    the sign.  The slices are read as unsigned by every call they go into, so a predicate on the difference names
    the sign beside it: `a - b <= c` for c >= 0 is `0 <= diff <= c AND a >= b` (a row with a < b has its top slice set and lies
    far above c) --
        diff = subtract_columns(wah, a, b)
        filter_columns(wah, [(*range_column(wah, diff, 0, c), [0], False), (*compare_columns(wah, a, ">=", b), [0], False)], n)
    -- and `a - b < 0` is compare_columns(wah, a, "<", b), or the top slice itself."""
    return _arith_columns(wah, "-", bsi_a, bsi_b, n_bits, table, reuse)


def multiply_columns(wah, bsi_a, bsi_b, n_bits=None, table=None, **reuse):
    """`A * B` row by row over TWO bit-sliced attributes in one call, as a NEW bit-sliced attribute (wah_bsi_mul_indexed_device):
    arguments and result as add_columns.  The result holds (A * B) mod 2^n_bits, both values read as unsigned; n_bits defaults
    to min(ka + kb, 63), which loses nothing below 63 bits (the call itself takes 1 .. 64).  The operation is commutative and the
    call keeps an image of its first operand in the scratch, so the NARROWER attribute is passed as A (bsi_a where the widths
    are equal); multiply_columns(a, b) and multiply_columns(b, a) return the same streams.  The table
    puts the existence rows first, then all of A's slices, then all of B's, least significant first (api.bsi_mul_row_order); a
    table passed in is overwritten in that order."""
    import torch

    from . import api

    if bsi_b[3] < bsi_a[3]:
        bsi_a, bsi_b = bsi_b, bsi_a
    _, _, n, ka, has_a = bsi_a
    _, _, n_b, kb, has_b = bsi_b
    if n != n_b:
        raise ValueError("the two attributes have different column lengths")
    n_bits = min(ka + kb, 63) if n_bits is None else int(n_bits)
    if not 1 <= n_bits <= 64:
        raise ValueError("between 1 and 64 bits")
    table = _two_attribute_table(wah.bsi_mul_row_order(ka, kb, has_a, has_b), bsi_a, bsi_b, table)
    has_exists = bool(has_a or has_b)
    flags = (wah.BSI_EXISTS_A if has_a else 0) | (wah.BSI_EXISTS_B if has_b else 0)
    check = reuse.pop("check", True)
    if reuse.get("scratch") is None:
        reuse["scratch"] = torch.empty(int(wah.lib().wah_bsi_mul_scratch_bytes(n, ka, n_bits, flags)), dtype=torch.uint8, device=table.device)
    out, count, out_offsets = wah.bsi_mul_device(table, ka, kb, n_bits, n, exists_a=has_a, exists_b=has_b, check=False, **reuse)
    if not check:
        return out, out_offsets, n, n_bits, has_exists
    api._check(wah.lib().wah_bsi_mul_status(reuse["scratch"].data_ptr(), n, ka, n_bits, flags, api._stream_ptr(torch)), "bsi_mul")
    return out[: int(count.item())], out_offsets, n, n_bits, has_exists


def _div_columns(wah, remainder, bsi_a, bsi_b, n_bits, table, reuse):
    """divide_columns / modulo_columns: one wah_bsi_div_indexed_device call over two bsi_from_values results, operands as given."""
    import torch

    from . import api

    _, _, n, ka, has_a = bsi_a
    _, _, n_b, kb, has_b = bsi_b
    if n != n_b:
        raise ValueError("the two attributes have different column lengths")
    n_bits = (min(ka, kb) if remainder else ka) if n_bits is None else int(n_bits)
    if not 1 <= n_bits <= 64:
        raise ValueError("between 1 and 64 bits")
    table = _two_attribute_table(wah.bsi_div_row_order(ka, kb, has_a, has_b), bsi_a, bsi_b, table)
    flags = (wah.BSI_EXISTS_A if has_a else 0) | (wah.BSI_EXISTS_B if has_b else 0)
    check = reuse.pop("check", True)
    if reuse.get("scratch") is None:
        reuse["scratch"] = torch.empty(int(wah.lib().wah_bsi_div_scratch_bytes(n, kb, n_bits, flags)), dtype=torch.uint8, device=table.device)
    out, count, out_offsets = wah.bsi_div_device(table, ka, kb, n_bits, n, remainder=remainder, exists_a=has_a, exists_b=has_b, check=False, **reuse)
    if not check:
        return out, out_offsets, n, n_bits, True
    api._check(wah.lib().wah_bsi_div_status(reuse["scratch"].data_ptr(), n, kb, n_bits, flags, api._stream_ptr(torch)), "bsi_div")
    return out[: int(count.item())], out_offsets, n, n_bits, True


def divide_columns(wah, bsi_a, bsi_b, n_bits=None, table=None, **reuse):
    """`A / B` row by row over TWO bit-sliced attributes in one call, as a NEW bit-sliced attribute (wah_bsi_div_indexed_device):
    arguments and result as add_columns.  The result holds floor(A / B) mod 2^n_bits, both values read as unsigned; n_bits
    defaults to ka, which loses nothing.  A division by zero is NULL: the result ALWAYS has an existence bitmap (has_exists is
    True), the AND of those the operands have and of B != 0, and a row outside it is stored as 0.  The operands are taken as
    given.  The table puts the existence rows first, then all of B's slices, least significant first, then all of A's, most
    significant first (api.bsi_div_row_order); a table passed in is overwritten in that order."""
    return _div_columns(wah, False, bsi_a, bsi_b, n_bits, table, reuse)


def modulo_columns(wah, bsi_a, bsi_b, n_bits=None, table=None, **reuse):
    """`A % B` row by row, arguments and result as divide_columns.  The result holds (A mod B) mod 2^n_bits; n_bits defaults to
    min(ka, kb), which loses nothing.  Its existence bitmap is that of the quotient, so A == Q * B + R holds in exactly the rows
    both have."""
    return _div_columns(wah, True, bsi_a, bsi_b, n_bits, table, reuse)


def divide_column_by(wah, bsi, c, remainder=False, n_bits=None):
    """`value / c`, or with remainder=True `value % c`, for a Python int 1 <= c < 2^63: divide_columns / modulo_columns by a
    constant attribute of c.bit_length() slices built with bsi_from_values from a full column -- each of its slices is one fill
    per segment.  Result as divide_columns; ValueError for c < 1."""
    import torch

    c = int(c)
    if not 1 <= c < (1 << 63):
        raise ValueError("a divisor between 1 and 2^63 - 1")
    n = bsi[2]
    constant = bsi_from_values(wah, torch.full((32 * n,), c, dtype=torch.int64, device=bsi[0].device), c.bit_length(), n_words_per_column=n)
    return (modulo_columns if remainder else divide_columns)(wah, bsi, constant, n_bits=n_bits)


def sum_product_where(wah, bsi_a, bsi_b, mask_stream, mask_offsets):
    """`SELECT SUM(a * b) WHERE <mask>` over two bit-sliced attributes: multiply_columns with all ka + kb slices, then
    sum_column_where over the product.  Raises ValueError where ka + kb > 64: the product would be truncated.  Returns a
    Python int."""
    ka, kb = bsi_a[3], bsi_b[3]
    if ka + kb > 64:
        raise ValueError("the product of the two attributes needs more than 64 bits")
    return sum_column_where(wah, multiply_columns(wah, bsi_a, bsi_b, n_bits=ka + kb), mask_stream, mask_offsets)


def sum_column_where(wah, bsi, mask_stream, mask_offsets):
    """`SELECT SUM(value) WHERE <mask>` over a bit-sliced attribute without decoding a bitmap: ONE wah_count_masked_indexed_device
    call with the mask (an indexed compressed bitmap of the attribute's column length: a filter_columns or range_column result)
    as the one mask row and the slices as operands, then sum(count[i] << significance of slice i) in Python ints, which do not
    overflow.  Rows outside an existence bitmap were stored as 0 and add nothing.  Returns a Python int."""
    stream, seg_offsets, n, n_bits, _ = bsi
    slices = column_operand_table(stream, seg_offsets, n, list(range(n_bits)))
    counts = wah.count_masked_device([(mask_stream, mask_offsets)], slices, n).view(-1).tolist()
    return sum(int(cnt) << (n_bits - 1 - i) for i, cnt in enumerate(counts))


def _group_tables(wah, keys, n_words_per_column, where):
    """The tables a grouped call ANDs: (filter table [F, 3] or None, group table [G, R, 3], the keys' column counts).  The groups
    are the Cartesian product of the keys' columns in row-major order, made by indexing on the device."""
    import torch

    n = int(n_words_per_column)
    if not 1 <= len(keys) <= 8:
        raise ValueError("between 1 and 8 grouping attributes")
    tables = [column_operand_table(stream, seg_offsets, n, ids) for stream, seg_offsets, ids in keys]
    shape = tuple(int(t.shape[0]) for t in tables)
    dev = tables[0].device
    picks = torch.cartesian_prod(*[torch.arange(k, device=dev) for k in shape]).view(-1, len(keys))
    groups = torch.stack([t[picks[:, r]] for r, t in enumerate(tables)], dim=1).contiguous()
    if where is None:
        where = []
    elif isinstance(where, tuple):
        where = [where]
    return (wah.bitop_operand_table(list(where)) if len(where) else None), groups, shape


def aggregate_columns(wah, keys, attributes, n_words_per_column, where=None, **reuse):
    """`SELECT g, h, COUNT(*), SUM(x), COUNT(x), SUM(y) WHERE <where> GROUP BY g, h` in ONE call that decodes no bitmap, writes
    none and finishes nothing on the host (wah_group_sum_indexed_device).  keys: a list of 1 .. 8 (stream, seg_offsets, column_ids)
    of equality-encoded attributes (compress_column_matrix / index_from_keys results; arguments as column_operand_table): the
    groups are the Cartesian product of their columns, row-major.  attributes: a list of bsi_from_values / add_columns /
    subtract_columns / multiply_columns results of the same column length; one that has an existence bitmap gets that bitmap as
    one more attribute of 1 bit, whose "sum" is COUNT(value) (rows outside it were stored as 0 and add nothing to the sum).
    where: None, one (stream, seg_offsets) pair or a list of them -- filter_columns / range_column / compare_columns results --,
    all ANDed.  reuse: scratch / group_rows / counts / sums / check of api.group_sum_device.  Returns a dict:
      rows:   int64 device tensor shaped by the keys' column counts: COUNT(*) per group;
      sums:   per attribute an object array of that shape of Python ints, low + (high << 64): SUM(value);
      counts: per attribute COUNT(value) as an int64 device tensor of that shape: the existence count, or `rows` itself where
              the attribute has no existence bitmap.
    AVG(value) is sums / counts wherever counts is not 0; it is not computed here."""
    import numpy as np
    import torch

    n = int(n_words_per_column)
    if not attributes:
        raise ValueError("at least one attribute")
    filters, groups, shape = _group_tables(wah, keys, n, where)
    parts, bits, places = [], [], []  # places: (the attribute's place in attr_bits, its existence bitmap's or None)
    for stream, seg_offsets, n_attr, n_bits, has_exists in attributes:
        if n_attr != n:
            raise ValueError("the attributes' columns are as long as the keys'")
        parts.append(column_operand_table(stream, seg_offsets, n, list(range(n_bits + (1 if has_exists else 0)))))
        places.append((len(bits), len(bits) + 1 if has_exists else None))
        bits += [n_bits, 1] if has_exists else [n_bits]
    if len(bits) > wah.GROUP_MAX_ATTRS:
        raise ValueError("at most 64 attributes, existence bitmaps included")
    rows, _, sums = wah.group_sum_device(filters, groups.view(-1, 3), torch.cat(parts), bits, n, rows_per_group=len(keys), **reuse)
    rows = rows.view(shape)
    words = sums.cpu().numpy().astype(object) & ((1 << 64) - 1)
    whole = (words[:, :, 0] + (words[:, :, 1] << 64)).reshape(shape + (len(bits),))
    return {"rows": rows,
            "sums": [np.ascontiguousarray(whole[..., at]) for at, _ in places],
            "counts": [rows if ex is None else sums[:, ex, 0].reshape(shape) for _, ex in places]}


GROUP_BY_DROP = 0xFFFFFFFF  # a lookup entry that no bucket count reaches: the key's rows go to "other"


def _lookup_tensor(lookup, dev):
    """A key -> bucket table as the contiguous int32 device tensor the call reads (bit patterns: 0xFFFFFFFF is -1)."""
    import torch

    if not torch.is_tensor(lookup):
        lookup = torch.as_tensor(lookup, dtype=torch.int64)
    if lookup.dtype not in (torch.int32, torch.uint32):
        low = lookup.to(torch.int64) & 0xFFFFFFFF
        lookup = ((low ^ 0x80000000) - 0x80000000).to(torch.int32)  # the low 32 bits as the int32 of the same pattern
    return lookup.to(dev).reshape(-1).contiguous()


def group_by_column(wah, key, n_rows, attributes=(), where=None, lookup=None, n_buckets=None):
    """`SELECT key, COUNT(*), SUM(x), COUNT(x), SUM(y) WHERE <where> GROUP BY key` where the key is a BIT-SLICED attribute of up
    to 32 bits -- a customer id, a date key -- with one wah_bsi_group_by_indexed_device call per attribute piece and no value
    column, decoded filter or bitmap in between.  key: a bsi_from_values result (rows outside its existence bitmap are in no
    bucket); n_rows: the table's rows, at most 32 * the column length; attributes: bsi_from_values / add_columns / ... results of
    the key's column length -- one wider than 32 slices goes as two calls over its low and high slices, combined as
    hi << 32 | lo in Python ints, and one with an existence bitmap gets that bitmap as one more attribute of 1 slice, whose
    sum is COUNT(value); where: None, one (stream, seg_offsets) pair or a list of them, all ANDed; lookup: key -> bucket (a device
    tensor or a sequence of ints; a key at or behind its end, and an entry at or above n_buckets such as GROUP_BY_DROP, go to
    "other"), or None: the key is the bucket; n_buckets defaults to 2 ** n_bits of the key, or to the largest lookup entry that
    is not GROUP_BY_DROP, plus one (read back).  Returns a dict shaped like aggregate_columns':
      rows:   int64 device tensor [n_buckets]: COUNT(*) per bucket;
      sums:   per attribute an object array [n_buckets] of Python ints, low + (high << 64): SUM(value);
      counts: per attribute COUNT(value) as an int64 device tensor [n_buckets]: `rows` itself without an existence bitmap;
      other:  the same three for the bucket "other": {"rows": int, "sums": [int], "counts": [int]}."""
    import numpy as np
    import torch

    stream, seg_offsets, n, n_bits, has_exists = key
    if n_bits > 32:
        raise ValueError("a key of at most 32 slices: bucket its low slices, or group after subtract_columns / range_column")
    dev = stream.device
    key_table = _slice_table(key)
    if where is None:
        where = []
    elif isinstance(where, tuple):
        where = [where]
    filters = wah.bitop_operand_table(list(where)) if len(where) else None
    if lookup is not None:
        lookup = _lookup_tensor(lookup, dev)
    if n_buckets is None:
        if lookup is None:
            n_buckets = 1 << n_bits
        else:
            wide = lookup.to(torch.int64) & 0xFFFFFFFF
            n_buckets = int(torch.where(wide == GROUP_BY_DROP, torch.full_like(wide, -1), wide).max().item()) + 1
    b = max(int(n_buckets), 1)

    def call(table):
        return wah.bsi_group_by_device(key_table, n, n_rows, b, value_table=table, filters=filters, exists=has_exists, lookup=lookup)

    def whole(sums, shift=0):  # [b + 1, 2] int64 -> Python ints
        words = sums.cpu().numpy().astype(object) & ((1 << 64) - 1)
        return (words[:, 0] + (words[:, 1] << 64)) << shift

    rows, all_sums, all_counts = None, [], []
    for a_stream, a_offsets, n_attr, a_bits, a_exists in attributes:
        if n_attr != n:
            raise ValueError("the attributes' columns are as long as the key's")
        ids = list(range(a_bits))
        low = column_operand_table(a_stream, a_offsets, n, ids[-32:])
        rows, sums = call(low)
        total = whole(sums)
        if a_bits > 32:
            total = total + whole(call(column_operand_table(a_stream, a_offsets, n, ids[:-32]))[1], 32)
        all_sums.append(total)
        all_counts.append(call(column_operand_table(a_stream, a_offsets, n, [a_bits]))[1][:, 0].contiguous() if a_exists else rows)
    if rows is None:
        rows = call(None)[0]
    return {"rows": rows[:b],
            "sums": [np.ascontiguousarray(s[:b]) for s in all_sums],
            "counts": [c[:b] for c in all_counts],
            "other": {"rows": int(rows[b]), "sums": [int(s[b]) for s in all_sums], "counts": [int(c[b]) for c in all_counts]}}


def group_by_joined(wah, fk, n_rows, dim_groups, dim_keep=None, attributes=(), where=None, n_buckets=None):
    """The star join's GROUP BY in the fact table's index: `SELECT d.g, COUNT(*), SUM(f.x) FROM f JOIN d ON f.fk = d.rowid WHERE
    <d filter> AND <where> GROUP BY d.g`.  fk: the fact table's foreign key, a ROW NUMBER of the dimension table, as a bit-sliced
    attribute; dim_groups: an integer device tensor with the group of every dimension row; dim_keep: a bool device tensor, the
    dimension rows the dimension's filter keeps, or None: all.  The lookup is built on the device -- dim_groups where dim_keep,
    else GROUP_BY_DROP -- and group_by_column does the rest: fact rows whose dimension row is filtered out, or lies behind the
    dimension table, are in "other".  n_buckets defaults to the largest group + 1 (read back).  Returns group_by_column's dict."""
    import torch

    groups = dim_groups.reshape(-1).to(torch.int64)
    if n_buckets is None:
        n_buckets = int(groups.max().item()) + 1 if groups.numel() else 1
    if dim_keep is not None:
        groups = torch.where(dim_keep.reshape(-1), groups, torch.full_like(groups, GROUP_BY_DROP))
    return group_by_column(wah, fk, n_rows, attributes=attributes, where=where, lookup=groups, n_buckets=n_buckets)


MAP_NULL = 0xFFFFFFFF  # a lookup entry without a value (WAH_MAP_NULL): 2^32 - 1 is therefore not a storable value


def map_column(wah, key, n_rows, lookup, n_bits=None, partial=False, **reuse):
    """A bit-sliced key pushed through a lookup table, as a NEW bit-sliced attribute of the same table, in one call
    (wah_bsi_map_indexed_device): no value column is read out, gathered and built again.  key: a bsi_from_values result of at most
    32 slices; n_rows: the table's rows, at most 32 * the column length; lookup: key -> value, a device tensor or a sequence of
    ints, MAP_NULL (-1 as int32) for "no value" -- an int32 / uint32 device tensor is read in place by the device only, which is
    what a captured graph replayed over a rewritten lookup needs.  n_bits: the result's width, 1 .. 32; it defaults to the width of
    the largest entry that is not MAP_NULL (read back once), at least 1.  A row has a value when it lies in front of n_rows, is in
    the key's existence bitmap, its key lies inside the lookup and its entry is not MAP_NULL.  partial=False: every other existing
    row in front of n_rows is an error (WahError from the status, as an entry wider than n_bits is in either mode);
    partial=True: such a row has no value -- it is stored as 0 and lies outside the result's existence bitmap.  The result has
    an existence bitmap when the key has one or partial is set.  reuse: scratch / out / out_offsets / check of api.bsi_map_device.
    Returns the five-tuple of bsi_from_values (stream, seg_offsets, n_words_per_column, n_bits, has_exists), which goes into
    compare_columns, multiply_columns, group_by_column, kth_column_where, range_column and another map_column as it is;
    check=False reads nothing back and returns the whole output buffer, as there.
    The call is measured against the road it replaces -- values_of_column, lookup[values] in torch, bsi_from_values -- by
    tools/bsi_map_time.py (profiles/bsi_map_time.txt): at 2^24 rows, keys of 12 and 24 bits, lookups of 4 Ki and
    16 Mi entries, results of 8 and 32 bits, uniform and sorted keys it took 0.20 .. 0.59 ms against 0.27 .. 0.69 ms -- ahead by
    1.1 to 1.2 times at seven of the eight shapes, within the spread at one, slower at none, and far from the 2.5 to 5 times
    fewer bytes it moves."""
    import torch

    from . import api

    stream, _, n, key_bits, key_exists = key
    if key_bits > 32:
        raise ValueError("a key of at most 32 slices")
    lookup = _lookup_tensor(lookup, stream.device)
    if n_bits is None:
        wide = lookup.to(torch.int64) & 0xFFFFFFFF
        n_bits = max(int(torch.where(wide == MAP_NULL, torch.zeros_like(wide), wide).max().item()).bit_length(), 1) if lookup.numel() else 1
    n_bits = int(n_bits)
    if not 1 <= n_bits <= 32:
        raise ValueError("between 1 and 32 bits")
    has_exists = bool(key_exists or partial)
    flags = (wah.BSI_EXISTS if key_exists else 0) | (wah.MAP_PARTIAL if partial else 0)
    check = reuse.pop("check", True)
    if reuse.get("scratch") is None:
        reuse["scratch"] = torch.empty(int(wah.lib().wah_bsi_map_scratch_bytes(n, n_bits, flags)), dtype=torch.uint8, device=stream.device)
    out, count, out_offsets = wah.bsi_map_device(_slice_table(key), n, n_rows, lookup, n_bits, exists=bool(key_exists), partial=partial, check=False,
                                                 **reuse)
    if not check:
        return out, out_offsets, n, n_bits, has_exists
    api._check(wah.lib().wah_bsi_map_status(reuse["scratch"].data_ptr(), n, n_bits, flags, api._stream_ptr(torch)), "bsi_map")
    return out[: int(count.item())], out_offsets, n, n_bits, has_exists


def join_column(wah, fk, n_rows, dim_values, dim_keep=None, n_bits=None):
    """The star join's PROJECTION in the fact table's index: `SELECT d.x FROM f JOIN d ON f.fk = d.rowid [WHERE <d filter>]` as a
    bit-sliced attribute of f, one map_column call.  fk: the fact table's foreign key, a ROW NUMBER of the dimension table, as a
    bit-sliced attribute; dim_values: an integer device tensor with d.x of every dimension row (a values_of_column result of the
    dimension, for example), below 2^32 - 1; dim_keep: a bool device tensor, the dimension rows the dimension's filter keeps, or
    None: all.  The lookup is built on the device -- dim_values where dim_keep, else MAP_NULL -- and the call is always partial: a
    fact row whose dimension row is filtered out, or lies behind the dimension table, has no value and lies outside the result's
    existence bitmap.  n_bits: as map_column.  Returns map_column's five-tuple."""
    import torch

    values = dim_values.reshape(-1).to(torch.int64)
    if dim_keep is not None:
        values = torch.where(dim_keep.reshape(-1), values, torch.full_like(values, MAP_NULL))
    return map_column(wah, fk, n_rows, values, n_bits=n_bits, partial=True)


def apply_column(wah, key, n_rows, fn, n_bits=None):
    """A unary function of a bit-sliced key as a new bit-sliced attribute -- `EXTRACT(year FROM date_key)`, `price // 10`, a CASE,
    histogram bins: fn is tabulated ONCE over the key's domain and the table goes through map_column.  fn is called once with
    torch.arange(2 ** key_bits) on the key's device and returns an integer tensor of that length, its values below 2^32 - 1; a
    NEGATIVE result means NULL.  The call is always partial (a row whose result is NULL has no value), so the result always has
    an existence bitmap.  A key of more than 24 slices is refused: its table would be 64 MiB and more -- build the lookup
    yourself and use map_column.  n_bits: as map_column.  Returns map_column's five-tuple."""
    import torch

    key_bits = key[3]
    if key_bits > 24:
        raise ValueError("a key of at most 24 slices: build the lookup yourself and use map_column")
    result = fn(torch.arange(1 << key_bits, dtype=torch.int64, device=key[0].device)).reshape(-1).to(torch.int64)
    if result.numel() != 1 << key_bits:
        raise ValueError("fn returns one result per key of the domain")
    return map_column(wah, key, n_rows, torch.where(result < 0, torch.full_like(result, MAP_NULL), result), n_bits=n_bits, partial=True)


def _cumsum(wah, val_table, n, n_rows, val_bits, n_bits, filters, exists, exclusive, all_rows, dev, reuse):
    """cumsum_column's and row_numbers_where's call: api.bsi_cumsum_device with a scratch of its own, the five-tuple back."""
    import torch

    from . import api

    flags = (wah.BSI_EXISTS if exists else 0) | (wah.CUMSUM_EXCLUSIVE if exclusive else 0) | (wah.CUMSUM_ALL_ROWS if all_rows else 0)
    check = reuse.pop("check", True)
    if reuse.get("scratch") is None:
        reuse["scratch"] = torch.empty(int(wah.lib().wah_bsi_cumsum_scratch_bytes(n, n_bits, flags)), dtype=torch.uint8, device=dev)
    out, count, out_offsets = wah.bsi_cumsum_device(val_table, n, n_rows, val_bits, n_bits, filters=filters, exists=exists, exclusive=exclusive,
                                                    all_rows=all_rows, check=False, **reuse)
    if not check:
        return out, out_offsets, n, n_bits, not all_rows
    api._check(wah.lib().wah_bsi_cumsum_status(reuse["scratch"].data_ptr(), n, n_bits, flags, api._stream_ptr(torch)), "bsi_cumsum")
    return out[: int(count.item())], out_offsets, n, n_bits, not all_rows


def _where_list(where):
    return [] if where is None else [where] if isinstance(where, tuple) else list(where)


def cumsum_column(wah, bsi, n_rows, where=None, exclusive=False, all_rows=False, n_bits=None, **reuse):
    """`SELECT SUM(x) OVER (ORDER BY rowid) FROM t WHERE <where>`: the running total of a bit-sliced attribute over the selected
    rows, as a NEW bit-sliced attribute of the same table, in one call (wah_bsi_cumsum_indexed_device): no value column is read
    out, scanned and built again.  bsi: a bsi_from_values result of at most 32 slices, unsigned; n_rows: the table's rows, at most
    32 * the column length; where: None, one (stream, seg_offsets) pair or a list of them, all ANDed.  A row is selected when it
    lies in front of n_rows, is in every `where` bitmap and in the attribute's existence bitmap, if it has one.  Row p of the
    result holds the sum of the values of the selected rows up to and including p (exclusive=True: in front of p), mod
    2^n_bits; n_bits, 1 .. 64, defaults to min(64, the attribute's width + bit_length(n_rows)), which no sum of n_rows such
    values passes.  all_rows=False: only the selected rows hold a value, every other row is stored as 0 and lies outside the
    result's existence bitmap, which is the selection; all_rows=True: every row in front of n_rows holds the running value and the
    result has no existence bitmap.  reuse: scratch / out / out_offsets / check of api.bsi_cumsum_device.  Returns the five-tuple of
    bsi_from_values (stream, seg_offsets, n_words_per_column, n_bits, has_exists), which goes into range_column, compare_columns,
    kth_column_where, values_of_column and another cumsum_column (one of at most 32 slices) as it is; check=False reads nothing
    back and returns the whole output buffer, as map_column does.
    The call is measured against the road it replaces -- values_of_column, torch.cumsum, bsi_from_values -- by
    tools/bsi_cumsum_time.py (profiles/bsi_cumsum_time.txt): at 2^24 rows, values of 8 and 32 bits, results of 32
    and 56 slices, without a filter and under a filter of one half of the rows, its median of seven runs was 0.35 .. 0.57 ms
    against 0.54 .. 0.71 ms -- ahead by 1.24 to 1.56 times by the medians, at seven of the eight shapes by more than the spread
    and at one (8 bits to 32 slices, no filter) within it, slower at none; the lead shrinks as the result widens."""
    stream, seg_offsets, n, val_bits, val_exists = bsi
    if val_bits > 32:
        raise ValueError("a value of at most 32 slices")
    if n_bits is None:
        n_bits = min(64, val_bits + int(n_rows).bit_length())
    n_bits = int(n_bits)
    if not 1 <= n_bits <= 64:
        raise ValueError("between 1 and 64 bits")
    where = _where_list(where)
    filters = wah.bitop_operand_table(where) if len(where) else None
    return _cumsum(wah, _slice_table(bsi), n, n_rows, val_bits, n_bits, filters, bool(val_exists), exclusive, all_rows, stream.device, reuse)


def row_numbers_where(wah, where, n_words_per_column, n_rows, exclusive=False, all_rows=False, **reuse):
    """`SELECT ROW_NUMBER() OVER (ORDER BY rowid) FROM t WHERE <where>` as a bit-sliced attribute: the running COUNT of the rows
    that `where` selects, wah_bsi_cumsum_indexed_device without value slices.  where: one (stream, seg_offsets) pair or a list of
    them (at least one), all ANDed; n_rows: the table's rows, at most 32 * n_words_per_column; the result has bit_length(n_rows)
    slices, at least 1.  With the defaults every selected row holds its number among the selected rows, from 1 on, and the
    result's existence bitmap is the selection.  exclusive=True, all_rows=True: EVERY row in front of n_rows holds the number of
    selected rows in front of it -- the destination rank that keep_rows moves a row to -- and the result has no existence bitmap.
    reuse and the returned five-tuple as cumsum_column's."""
    where = _where_list(where)
    if not len(where):
        raise ValueError("at least one filter bitmap")
    n_bits = max(int(n_rows).bit_length(), 1)
    return _cumsum(wah, None, int(n_words_per_column), n_rows, 0, n_bits, wah.bitop_operand_table(where), False, exclusive, all_rows,
                   where[0][0].device, reuse)


def _cumsum_by(wah, val_table, n, n_rows, val_bits, n_bits, starts, filters, exists, exclusive, all_rows, dev, reuse):
    """cumsum_column_by's and row_numbers_by's call: _cumsum with the starts row, api.bsi_cumsum_parts_device."""
    import torch

    from . import api

    flags = (wah.BSI_EXISTS if exists else 0) | (wah.CUMSUM_EXCLUSIVE if exclusive else 0) | (wah.CUMSUM_ALL_ROWS if all_rows else 0)
    check = reuse.pop("check", True)
    if reuse.get("scratch") is None:
        reuse["scratch"] = torch.empty(int(wah.lib().wah_bsi_cumsum_parts_scratch_bytes(n, n_bits, flags)), dtype=torch.uint8, device=dev)
    out, count, out_offsets = wah.bsi_cumsum_parts_device(val_table, n, n_rows, val_bits, n_bits, starts, filters=filters, exists=exists,
                                                          exclusive=exclusive, all_rows=all_rows, check=False, **reuse)
    if not check:
        return out, out_offsets, n, n_bits, not all_rows
    api._check(wah.lib().wah_bsi_cumsum_parts_status(reuse["scratch"].data_ptr(), n, n_bits, flags, api._stream_ptr(torch)), "bsi_cumsum_parts")
    return out[: int(count.item())], out_offsets, n, n_bits, not all_rows


def _starts_pair(starts):
    """starts as api.bsi_cumsum_parts_device takes it: a (stream, seg_offsets) pair, also the first two of a longer result tuple."""
    return tuple(starts[:2]) if isinstance(starts, tuple) else starts


def cumsum_column_by(wah, bsi, n_rows, starts, where=None, exclusive=False, all_rows=False, n_bits=None, **reuse):
    """`SELECT SUM(x) OVER (PARTITION BY g ORDER BY rowid) FROM t WHERE <where>` on a table clustered by g (reorder_rows): cumsum_column
    with a sum that starts again at every row of `starts`, in one call (wah_bsi_cumsum_parts_indexed_device).  starts: the bitmap
    of the partitions' first rows, a (stream, seg_offsets) pair -- partition_starts makes it from the key -- or a one-row operand
    table; a row starts a partition whether or not it is selected, row 0 needs no bit.  Row p of the result holds the sum of the
    values of the selected rows from its partition's first row up to and including p (exclusive=True: in front of p); with
    all_rows=True an unselected row carries its partition's running value.  bsi, n_rows, where, n_bits (the same default: no
    partition's sum passes the whole table's), reuse and the returned five-tuple as cumsum_column's.
    Timed against the road it replaces -- values_of_column, a segmented cumsum in torch, bsi_from_values -- and against
    cumsum_column by tools/bsi_cumsum_parts_time.py (profiles/bsi_cumsum_parts_time.txt): at 2^24 rows, partitions
    of about 2^16 and of about 16 rows, its median of seven runs was 0.40 .. 0.67 ms against 0.98 .. 1.20 ms, ahead by 1.8 to 2.5
    times at all eight shapes; against cumsum_column it is 4 to 12 per cent slower, at two shapes within the spread."""
    stream, seg_offsets, n, val_bits, val_exists = bsi
    if val_bits > 32:
        raise ValueError("a value of at most 32 slices")
    if n_bits is None:
        n_bits = min(64, val_bits + int(n_rows).bit_length())
    n_bits = int(n_bits)
    if not 1 <= n_bits <= 64:
        raise ValueError("between 1 and 64 bits")
    where = _where_list(where)
    filters = wah.bitop_operand_table(where) if len(where) else None
    return _cumsum_by(wah, _slice_table(bsi), n, n_rows, val_bits, n_bits, _starts_pair(starts), filters, bool(val_exists), exclusive, all_rows,
                      stream.device, reuse)


def row_numbers_by(wah, starts, n_words_per_column, n_rows, where=None, exclusive=False, all_rows=False, **reuse):
    """`SELECT ROW_NUMBER() OVER (PARTITION BY g ORDER BY rowid) FROM t [WHERE <where>]` as a bit-sliced attribute: the running COUNT
    of the selected rows within their partition, wah_bsi_cumsum_parts_indexed_device without value slices.  starts as
    cumsum_column_by's; where: None or empty (every row in front of n_rows), one (stream, seg_offsets) pair or a list of them, all
    ANDed.  The result has bit_length(n_rows) slices, at least 1.  exclusive, all_rows, reuse and the returned five-tuple as
    row_numbers_where's."""
    where = _where_list(where)
    starts = _starts_pair(starts)
    n_bits = max(int(n_rows).bit_length(), 1)
    dev = starts.device if hasattr(starts, "device") else starts[0].device
    return _cumsum_by(wah, None, int(n_words_per_column), n_rows, 0, n_bits, starts, wah.bitop_operand_table(where) if len(where) else None, False,
                      exclusive, all_rows, dev, reuse)


def partition_starts(wah, key, n_rows, shift=None, **reuse):
    """The bitmap of the rows p >= 1 (p < n_rows) whose key differs from row p - 1's: the partition starts of a table clustered by a
    bit-sliced key, composed on the device from two calls that decode nothing -- splice_columns of the key's row 0 and its rows
    0 .. n_rows - 2 is the key shifted down by one row, compare_columns(key, "!=", shifted) the starts.  key: a bsi_from_values
    result WITHOUT an existence bitmap (with one: ValueError -- whether a row without a value starts a partition is the caller's
    decision).  Row 0 needs no bit: a sum starts there anyway.  Where the key's columns hold rows at or behind n_rows, such a row
    is set if its key is not 0 -- the shifted key ends at n_rows -- which a call with the same n_rows does not see.  shift: a dict of splice_columns' reuse (source_words / scratch /
    out / out_offsets); reuse: table / scratch / out / out_offsets / check of compare_columns -- check=False enqueues both calls
    and reads nothing back, and the whole output buffer comes back.  Returns (stream, seg_offsets), which goes into
    cumsum_column_by and row_numbers_by as `starts`."""
    stream, seg_offsets, n, n_bits, has_exists = key
    n_rows = int(n_rows)
    if has_exists:
        raise ValueError("a key without an existence bitmap")
    if not 1 <= n_rows <= 32 * int(n):
        raise ValueError("between 1 and 32 * n_words_per_column rows")
    check = reuse.pop("check", True)
    matrix = (stream, seg_offsets, n)
    shifted, shifted_offsets, _ = splice_columns(wah, [(matrix, 0, 1), (matrix, 0, n_rows - 1)], n_words_per_column=n, check=check, **(shift or {}))
    got = compare_columns(wah, key, "!=", (shifted, shifted_offsets, n, n_bits, False), check=check, **reuse)
    return (got[0], got[-1])


def streak_lengths(wah, predicates_or_mask, n_words_per_column, n_rows):
    """For every row the mask selects the number of consecutive selected rows that end at it -- sessionisation, "gaps and
    islands": row_numbers_by with `where` the mask and `starts` its complement, which the clause call makes.
    predicates_or_mask: one (stream, seg_offsets) pair, or a list of filter_columns predicates, whose conjunction is the mask.
    Returns row_numbers_by's five-tuple: the streak's length so far in the selected rows, the mask as the existence bitmap."""
    n = int(n_words_per_column)
    mask = tuple(predicates_or_mask) if isinstance(predicates_or_mask, tuple) else filter_columns(wah, list(predicates_or_mask), n)
    gaps = wah.bitop_clauses_indexed_device([([mask], True)], n)
    return row_numbers_by(wah, gaps, n, n_rows, where=mask)


def _total_by(wah, val_table, n, n_rows, val_bits, n_bits, starts, filters, exists, all_rows, dev, reuse):
    """total_column_by's and partition_sizes' call: _cumsum_by for api.bsi_total_parts_device."""
    import torch

    from . import api

    flags = (wah.BSI_EXISTS if exists else 0) | (wah.CUMSUM_ALL_ROWS if all_rows else 0)
    check = reuse.pop("check", True)
    if reuse.get("scratch") is None:
        reuse["scratch"] = torch.empty(int(wah.lib().wah_bsi_total_parts_scratch_bytes(n, n_bits, flags)), dtype=torch.uint8, device=dev)
    out, count, out_offsets = wah.bsi_total_parts_device(val_table, n, n_rows, val_bits, n_bits, starts, filters=filters, exists=exists,
                                                         all_rows=all_rows, check=False, **reuse)
    if not check:
        return out, out_offsets, n, n_bits, not all_rows
    api._check(wah.lib().wah_bsi_total_parts_status(reuse["scratch"].data_ptr(), n, n_bits, flags, api._stream_ptr(torch)), "bsi_total_parts")
    return out[: int(count.item())], out_offsets, n, n_bits, not all_rows


def total_column_by(wah, bsi, n_rows, starts, where=None, all_rows=False, n_bits=None, **reuse):
    """`SELECT SUM(x) OVER (PARTITION BY g) FROM t WHERE <where>` on a table clustered by g: every row holds the TOTAL of its partition,
    in one call (wah_bsi_total_parts_indexed_device) -- the denominator of a share of total, the operand of a group mean, the
    subject of a HAVING brought back to rows.  starts as cumsum_column_by's; starts=None: no start, the grand total in every row
    (`SUM(x) OVER ()`).  Row p of the result holds the sum of the values of the selected rows of p's partition -- from the last
    start at or in front of p up to the row in front of the next start behind it --, mod 2^n_bits; all_rows=False: only selected
    rows hold it, the selection is the result's existence bitmap; all_rows=True: every row in front of n_rows holds it, a partition
    without a selected row 0, and there is no existence bitmap.  bsi, n_rows, where, n_bits (cumsum_column_by's default), reuse
    and the returned five-tuple as cumsum_column_by's.
    Timed against the road it replaces -- values_of_column, the partitions' totals and a gather back in torch, bsi_from_values -- and
    against cumsum_column_by by tools/bsi_total_parts_time.py (profiles/bsi_total_parts_time.txt): at 2^24 rows,
    values of 8 and 32 bits, results of 32 and 56 slices, partitions of about 2^16 and of about 16 rows, without a filter and under
    one of half the rows, its median of seven runs was 0.39 .. 0.71 ms against 0.87 .. 1.12 ms, ahead by 1.6 to 2.2 times at all
    eight shapes; against cumsum_column_by it is 3 to 9 per cent slower, at one shape within the spread."""
    stream, seg_offsets, n, val_bits, val_exists = bsi
    if val_bits > 32:
        raise ValueError("a value of at most 32 slices")
    if n_bits is None:
        n_bits = min(64, val_bits + int(n_rows).bit_length())
    n_bits = int(n_bits)
    if not 1 <= n_bits <= 64:
        raise ValueError("between 1 and 64 bits")
    where = _where_list(where)
    filters = wah.bitop_operand_table(where) if len(where) else None
    starts = _zero_bitmap(wah, n, stream.device) if starts is None else _starts_pair(starts)
    return _total_by(wah, _slice_table(bsi), n, n_rows, val_bits, n_bits, starts, filters, bool(val_exists), all_rows, stream.device, reuse)


def _zero_bitmap(wah, n, dev):
    """The indexed bitmap of n words without a set bit -- one zero fill per segment --, as a (stream, seg_offsets) pair."""
    import torch

    segs = int(n) // 992
    stream = torch.full((segs,), -(1 << 31) + 1024, dtype=torch.int32, device=dev)  # 0x80000400: a fill of 1024 groups of zeros
    return stream, torch.arange(segs + 1, dtype=torch.int64, device=dev)


def _sizes(wah, starts, n, n_rows, filters, all_rows, dev, reuse):
    """partition_sizes' and mean_column_by's call: _total_by without value slices under a filter TABLE (or None)."""
    n_bits = max(int(n_rows).bit_length(), 1)
    starts = _zero_bitmap(wah, n, dev) if starts is None else _starts_pair(starts)
    return _total_by(wah, None, int(n), n_rows, 0, n_bits, starts, filters, False, all_rows, dev, reuse)


def partition_sizes(wah, starts, n_words_per_column, n_rows, where=None, all_rows=False, **reuse):
    """`SELECT COUNT(*) OVER (PARTITION BY g) FROM t [WHERE <where>]` as a bit-sliced attribute: the number of selected rows of a
    row's partition, wah_bsi_total_parts_indexed_device without value slices.  starts as total_column_by's (a pair or a one-row
    table; None is not taken here: the device is the starts'); where: None or empty (every row in front of n_rows), one
    (stream, seg_offsets) pair or a list of them, all ANDed.  The result has bit_length(n_rows) slices, at least 1.  all_rows,
    reuse and the returned five-tuple as total_column_by's."""
    where = _where_list(where)
    starts = _starts_pair(starts)
    dev = starts.device if hasattr(starts, "device") else starts[0].device
    return _sizes(wah, starts, n_words_per_column, n_rows, wah.bitop_operand_table(where) if len(where) else None, all_rows, dev, reuse)


def mean_column_by(wah, bsi, n_rows, starts, where=None, all_rows=False):
    """`SELECT AVG(x) OVER (PARTITION BY g) FROM t WHERE <where>`, floored: divide_columns of total_column_by and of the number of
    selected rows of the partition -- the rows in front of n_rows that every `where` bitmap and the attribute's existence bitmap
    hold.  Two calls of wah_bsi_total_parts_indexed_device and one of wah_bsi_div_indexed_device, no new kernel.  The quotient
    always has an existence bitmap: a partition without a selected row is NULL (a division by zero), and with all_rows=False so
    is every row that is not selected.  Returns divide_columns' five-tuple, as wide as the attribute."""
    import torch

    stream, seg_offsets, n, val_bits, val_exists = bsi
    total = total_column_by(wah, bsi, n_rows, starts, where=where, all_rows=all_rows)
    where = _where_list(where)
    rows = [wah.bitop_operand_table(where)] if len(where) else []
    if val_exists:
        rows.append(column_operand_table(stream, seg_offsets, n, [val_bits]))
    size = _sizes(wah, starts, n, n_rows, torch.cat(rows) if rows else None, all_rows, stream.device, {})
    return divide_columns(wah, total, size, n_bits=max(val_bits, 1))


def rows_of_partitions_where(wah, bsi, n_rows, starts, op, bound, where=None):
    """`... WHERE g IN (SELECT g FROM t WHERE <where> GROUP BY g HAVING SUM(x) <op> <bound>)` brought back to rows: compare_column over
    total_column_by.  op: "<", "<=", ">", ">=" or "=="; bound: a Python int.  Returns (stream, seg_offsets) of the bitmap of the
    SELECTED rows -- in front of n_rows, in every `where` bitmap and in the attribute's existence bitmap -- whose partition's sum
    over the selected rows satisfies the comparison; a predicate for filter_columns, a mask for keep_rows."""
    return compare_column(wah, total_column_by(wah, bsi, n_rows, starts, where=where), op, bound)


def count_distinct_where(wah, key, n_rows, where=None):
    """`SELECT COUNT(DISTINCT key) WHERE <where>` over a bit-sliced key of up to 32 bits: the buckets of group_by_column that are
    not empty, counted on the device ("other" holds nothing without a lookup).  Returns an int64 device scalar."""
    return (group_by_column(wah, key, n_rows, where=where)["rows"] != 0).sum()


def extremes_by(wah, keys, bsi, n_words_per_column, where=None):
    """`SELECT g, h, MIN(value), MAX(value) WHERE <where> GROUP BY g, h` as plumbing over wah_bsi_kth_indexed_device, which ANDs
    its filter rows itself: per group TWO quantile calls (0/1 and 1/1) whose filters are the `where` rows, the group's own rows
    and the attribute's existence bitmap -- G x 2 calls, each with a host read of its result; no new kernel.  keys / where as
    aggregate_columns, bsi one bsi_from_values result of the same column length; at most 64 filter rows in all.  Returns
    (minima, maxima): two object arrays shaped by the keys' column counts, Python ints, None where no row of the group is
    selected."""
    import numpy as np
    import torch

    n = int(n_words_per_column)
    stream, seg_offsets, n_attr, n_bits, has_exists = bsi
    if n_attr != n:
        raise ValueError("the attribute's columns are as long as the keys'")
    filters, groups, shape = _group_tables(wah, keys, n, where)
    front = 0 if filters is None else int(filters.shape[0])
    n_filters = front + len(keys) + (1 if has_exists else 0)
    table = torch.empty((n_filters + n_bits, 3), dtype=torch.int64, device=stream.device)
    if filters is not None:
        table[:front] = filters
    column_operand_table(stream, seg_offsets, n, ([n_bits] if has_exists else []) + list(range(n_bits)), out=table[front + len(keys):])
    ends = [wah.bsi_kth_query(wah.BSI_KTH_QUANTILE, num, 1, device=stream.device) for num in (0, 1)]
    out = [np.empty(len(groups), dtype=object) for _ in ends]
    for g in range(len(groups)):
        table[front: front + len(keys)] = groups[g]
        for values, query in zip(out, ends):
            found, value = wah.bsi_kth_device(table, query, n, n_filters)[:2].tolist()
            values[g] = (value & ((1 << 64) - 1)) if found else None
    return out[0].reshape(shape), out[1].reshape(shape)


_QUANTILE_NAMES = {"min": (0, 1), "max": (1, 1), "median": (1, 2)}


def _quantile_queries(wah, queries):
    """(kind, a, b) triples of a quantiles_by query list: a triple stays, "min" / "max" / "median" and (num, den) become
    BSI_KTH_QUANTILE queries."""
    out = []
    for query in queries:
        if isinstance(query, str):
            if query not in _QUANTILE_NAMES:
                raise ValueError('a query is (kind, a, b), (num, den), "min", "max" or "median"')
            query = _QUANTILE_NAMES[query]
        query = tuple(int(v) for v in query)
        if len(query) == 2:
            num, den = query
            if den <= 0 or not 0 <= num <= den:
                raise ValueError("a quantile is num / den with 0 <= num <= den and den > 0")
            query = (wah.BSI_KTH_QUANTILE, num, den)
        if len(query) != 3:
            raise ValueError('a query is (kind, a, b), (num, den), "min", "max" or "median"')
        out.append(query)
    if not out:
        raise ValueError("at least one query")
    return out


def quantiles_by(wah, keys, bsi, n_words_per_column, queries, where=None, **reuse):
    """`SELECT g, h, MIN(value), MAX(value), median(value), ... WHERE <where> GROUP BY g, h` in ONE call that decodes no bitmap and
    writes none (wah_bsi_kth_grouped_indexed_device), with one host read, at the end.  keys / where as aggregate_columns (the
    groups are the Cartesian product of the keys' columns, row-major), bsi one bsi_from_values result of the same column length;
    its existence bitmap, when it has one, is one more filter (at most 64 filter rows in all).  queries: a list of (kind, a, b)
    triples as api.bsi_kth_query takes them, or the shorthands "min", "max", "median" and (num, den) for the quantile num / den;
    groups x queries <= 4096.  reuse: scratch / results / check of api.bsi_kth_grouped_device.  Returns a dict:
      values: an object array shaped by the keys' column counts + (Q,): Python ints in 0 .. 2^64 - 1, None where the query names
              no row of the group (an empty group, a rank beyond its rows);
      totals, less, equal: int64 device tensors of that shape: the group's selected rows, and those below / equal to the value.
    quantiles_by(..., ["min", "max"]) returns in values[..., 0] and values[..., 1] what extremes_by returns as its two arrays."""
    import numpy as np
    import torch

    n = int(n_words_per_column)
    stream, seg_offsets, n_attr, n_bits, has_exists = bsi
    if n_attr != n:
        raise ValueError("the attribute's columns are as long as the keys'")
    triples = _quantile_queries(wah, queries)
    filters, groups, shape = _group_tables(wah, keys, n, where)
    slices = column_operand_table(stream, seg_offsets, n, list(range(n_bits + (1 if has_exists else 0))))
    if has_exists:
        exists = slices[n_bits:]
        filters = exists if filters is None else torch.cat([filters, exists])
    results = wah.bsi_kth_grouped_device(filters, groups.view(-1, 3), slices[:n_bits], triples, n, rows_per_group=len(keys), **reuse)
    full = shape + (len(triples),)
    host = results.cpu().numpy().astype(object) & ((1 << 64) - 1)
    values = np.empty(host.shape[:2], dtype=object)
    for at in np.ndindex(*values.shape):
        values[at] = int(host[at][1]) if host[at][0] else None
    return {"values": values.reshape(full), "totals": results[:, :, 2].reshape(full), "less": results[:, :, 3].reshape(full),
            "equal": results[:, :, 4].reshape(full)}


def _kth_column(wah, bsi, query, mask, reuse):
    """One wah_bsi_kth_indexed_device call over a bsi_from_values result: the filters -- the mask, then the existence bitmap --
    in front of the slices.  Returns the five result words as Python ints in 0 .. 2^64 - 1."""
    import torch

    stream, seg_offsets, n, n_bits, has_exists = bsi
    ids = ([n_bits] if has_exists else []) + list(range(n_bits))
    n_mask = 0 if mask is None else 1
    table = torch.empty((n_mask + len(ids), 3), dtype=torch.int64, device=stream.device)
    if mask is not None:
        mask_stream, mask_offsets = mask
        table[0] = torch.tensor([mask_stream.data_ptr(), mask_stream.numel(), mask_offsets.data_ptr()], dtype=torch.int64)
    column_operand_table(stream, seg_offsets, n, ids, out=table[n_mask:])
    result = wah.bsi_kth_device(table, query, n, n_mask + (1 if has_exists else 0), **reuse)
    return [int(v) & ((1 << 64) - 1) for v in result.tolist()]


def kth_column_where(wah, bsi, k, mask=None, largest=False, **reuse):
    """The k-th smallest (largest=True: k-th largest) value, k counted from 0, of a bit-sliced attribute among the rows of a mask,
    in one call and without decoding a bitmap (wah_bsi_kth_indexed_device).  bsi: what bsi_from_values returned; mask: (stream,
    seg_offsets) of an indexed compressed bitmap of the attribute's column length -- a filter_columns or range_column result --
    or None for every row.  The attribute's existence bitmap, when it has one, is a filter too; without one every row of the
    column counts, those behind the caller's own with the value 0.  reuse: scratch / result of api.bsi_kth_device.  Returns
    (value, total): total the rows selected, value None when there are not more than k of them."""
    kind = wah.BSI_KTH_DESCENDING if largest else wah.BSI_KTH_ASCENDING
    found, value, total, _, _ = _kth_column(wah, bsi, (kind, int(k), 1), mask, reuse)
    return (value if found else None), total


def quantile_column_where(wah, bsi, num, den, mask=None, **reuse):
    """The value of rank floor(num * (total - 1) / den) from the bottom, 0 <= num <= den, den > 0: 0/1 the minimum, 1/2 the
    lower median, 99/100 the 99th percentile, 1/1 the maximum.  Arguments and result as kth_column_where; value is None when no
    row is selected."""
    num, den = int(num), int(den)
    if den <= 0 or not 0 <= num <= den:
        raise ValueError("a quantile is num / den with 0 <= num <= den and den > 0")
    found, value, total, _, _ = _kth_column(wah, bsi, (wah.BSI_KTH_QUANTILE, num, den), mask, reuse)
    return (value if found else None), total


def min_column_where(wah, bsi, mask=None, **reuse):
    """`SELECT MIN(value) WHERE <mask>`: quantile_column_where at 0/1."""
    return quantile_column_where(wah, bsi, 0, 1, mask, **reuse)


def max_column_where(wah, bsi, mask=None, **reuse):
    """`SELECT MAX(value) WHERE <mask>`: quantile_column_where at 1/1."""
    return quantile_column_where(wah, bsi, 1, 1, mask, **reuse)


def median_column_where(wah, bsi, mask=None, **reuse):
    """The lower median: quantile_column_where at 1/2."""
    return quantile_column_where(wah, bsi, 1, 2, mask, **reuse)


def top_rows(wah, bsi, k, mask=None, largest=True):
    """`SELECT rowid ... WHERE <mask> ORDER BY value DESC LIMIT k` (largest=False: ASC) as row numbers, without decoding a bitmap:
    the k-th value t is the threshold (wah_bsi_kth_indexed_device); the rows strictly beyond it are `value > t` (or `< t`) by
    range_column, ANDed with the mask by filter_columns and listed by api.positions_device; the rows of `value == t` fill up
    the rest, the first k - count of them in row order.  Plumbing over existing calls, with host reads of the result words in
    between.  Returns an int64 tensor of min(k, selected rows) row numbers: the strictly-better rows first, in row order,
    then the ties, in row order."""
    import torch

    stream, _, n, n_bits, _ = bsi
    k = int(k)
    empty = torch.empty(0, dtype=torch.int64, device=stream.device)
    if k <= 0:
        return empty
    kind = wah.BSI_KTH_DESCENDING if largest else wah.BSI_KTH_ASCENDING
    found, t, total, less, equal = _kth_column(wah, bsi, (kind, k - 1, 1), mask, {})
    if not found:
        if total == 0:
            return empty
        k = total  # fewer rows than asked for: all of them, the last one's value the threshold
        found, t, total, less, equal = _kth_column(wah, bsi, (kind, k - 1, 1), mask, {})
    better = total - less - equal if largest else less

    def rows_of(lo, hi, limit):
        got, offs = range_column(wah, bsi, lo, hi)
        if mask is not None:
            got, offs = filter_columns(wah, [(got, offs, [0], False), (mask[0], mask[1], [0], False)], n)
        return wah.positions_device(got, offs, n, limit=limit)[0]

    parts = []
    if better:
        parts.append(rows_of(t + 1, (1 << n_bits) - 1, better) if largest else rows_of(0, t - 1, better))
    parts.append(rows_of(t, t, k - better))
    return torch.cat(parts)


def _fetch_columns(wah, stream, seg_offsets, n_words_per_column, column_ids, rows, mode):
    """One wah_fetch_indexed_device call over columns of a compress_column_matrix result for rows in ANY order: the call wants
    them non-descending, so they are sorted (torch.sort) and the result is scattered back -- plumbing."""
    import torch

    if rows.dtype != torch.int64 or rows.dim() != 1 or rows.device != stream.device:
        raise ValueError("rows: a one-dimensional int64 tensor on the index's device")
    table = column_operand_table(stream, seg_offsets, n_words_per_column, column_ids)
    ordered, order = torch.sort(rows)
    got = wah.fetch_device(table, ordered.contiguous(), n_words_per_column, mode)
    out = torch.empty_like(got)
    out[order] = got
    return out


def values_at_rows(wah, bsi, rows):
    """`SELECT value ... WHERE rowid IN (rows)`: the values a bit-sliced attribute holds in the listed rows, in one call and
    without decoding a slice (wah_fetch_indexed_device, WAH_FETCH_BITS).  bsi: what bsi_from_values returned; rows: an int64
    device tensor of row numbers below 32 * n_words_per_column, in any order, duplicates allowed -- select_rows or top_rows
    output goes in as it is.  With an existence bitmap that bitmap is the table's first row, so the top bit of every fetched
    word says whether the row has a value.  Returns (values int64 tensor, have bool tensor or None), entry i for rows[i]."""
    stream, seg_offsets, n, n_bits, has_exists = bsi
    ids = ([n_bits] if has_exists else []) + list(range(n_bits))
    got = _fetch_columns(wah, stream, seg_offsets, n, ids, rows, wah.FETCH_BITS)
    if not has_exists:
        return got, None
    return got & ((1 << n_bits) - 1), ((got >> n_bits) & 1) != 0


def keys_at_rows(wah, index, rows):
    """The keys an equality-encoded attribute holds in the listed rows, in one call over ALL its value columns
    (wah_fetch_indexed_device, WAH_FETCH_FIRST): index is what index_from_keys returned, rows as for values_at_rows.  Returns
    an int64 tensor, entry i the key of rows[i], -1 where no column has the row (a row behind the key column's own length)."""
    stream, seg_offsets, n = index
    n_values = (int(seg_offsets.numel()) - 1) // (n // SEGMENT_WORDS)
    return _fetch_columns(wah, stream, seg_offsets, n, list(range(n_values)), rows, wah.FETCH_FIRST)


def _column_window(n_words_per_column, first, n_rows):
    """The window [first, first + n_rows) of a column as Python ints, n_rows defaulting to the rows behind `first`."""
    first = int(first)
    n_rows = 32 * int(n_words_per_column) - first if n_rows is None else int(n_rows)
    if first < 0 or n_rows < 0 or first + n_rows > 32 * int(n_words_per_column):
        raise ValueError("the window's rows lie inside the column")
    return first, n_rows


def values_of_column(wah, bsi, first=0, n_rows=None):
    """`SELECT value FROM t` over a row range: the values a bit-sliced attribute holds in rows [first, first + n_rows), in one call
    and without a decoded slice in global memory (wah_values_indexed_device, WAH_FETCH_BITS) -- the inverse of bsi_from_values
    at column scale: an export, an operand for torch, the input of a sort.  bsi: what bsi_from_values returned (or add_columns,
    multiply_columns, set_values_where ...); n_rows defaults to 32 * n_words_per_column - first.  The conventions are those of
    values_at_rows: with an existence bitmap that bitmap is the table's first row, its bit is masked off the values and returned
    as `have`.  Returns (values int64 tensor, have bool tensor or None), entry i for row first + i."""
    stream, seg_offsets, n, n_bits, has_exists = bsi
    first, n_rows = _column_window(n, first, n_rows)
    ids = ([n_bits] if has_exists else []) + list(range(n_bits))
    got = wah.values_device(column_operand_table(stream, seg_offsets, n, ids), n, wah.FETCH_BITS, first, n_rows)
    if not has_exists:
        return got, None
    return got & ((1 << n_bits) - 1), ((got >> n_bits) & 1) != 0


def keys_of_column(wah, index, first=0, n_rows=None):
    """The keys an equality-encoded attribute holds in rows [first, first + n_rows), in one call over ALL its value columns
    (wah_values_indexed_device, WAH_FETCH_FIRST) -- the inverse of index_from_keys.  index: what index_from_keys returned; the
    window as for values_of_column.  Returns an int64 tensor, -1 where no column has the row, as keys_at_rows does."""
    stream, seg_offsets, n = index
    first, n_rows = _column_window(n, first, n_rows)
    n_values = (int(seg_offsets.numel()) - 1) // (n // SEGMENT_WORDS)
    return wah.values_device(column_operand_table(stream, seg_offsets, n, list(range(n_values))), n, wah.FETCH_FIRST, first, n_rows)


def _values_of_column_torch(wah, bsi, first=0, n_rows=None):
    """values_of_column as it had to be done before wah_values_indexed_device, kept to be compared against (tools/values_time.py,
    the tests): every slice is decoded into the matrix [n_slices, n_words] (one wah_decompress_segments_device call) and the
    values are assembled with torch shifts and ORs, one slice after the other.  Arguments and result as values_of_column."""
    import torch

    stream, seg_offsets, n, n_bits, has_exists = bsi
    first, n_rows = _column_window(n, first, n_rows)
    k = n_bits + (1 if has_exists else 0)
    matrix = wah.decompress_segments_device(stream, seg_offsets, k * n)[: k * n].view(k, n)
    shifts = torch.arange(32, dtype=torch.int32, device=stream.device)

    def bits(row):  # the window's rows of one decoded bitmap as int64 0 / 1: position 32 * word + bit
        return ((matrix[row].view(n, 1) >> shifts) & 1).reshape(-1)[first: first + n_rows].to(torch.int64)

    values = torch.zeros(n_rows, dtype=torch.int64, device=stream.device)
    for i in range(n_bits):
        values |= bits(i) << (n_bits - 1 - i)
    return values, (bits(n_bits) != 0 if has_exists else None)


def reorder_rows(wah, index, order, n_rows):
    """Every column of an index rearranged together: row i of the result is row order[i] of the input -- ORDER BY over the whole
    table, clustering it by a sort key so that its bitmaps compress better, the gather of a join; it generalises slice_rows and
    keep_rows to any order.  index: the 3-tuple of index_from_keys or the 5-tuple of bsi_from_values, holding n_rows rows;
    order: an int64 device tensor in any order, repeats allowed, every entry in [0, n_rows).  Plumbing: the column is read with
    values_of_column / keys_of_column, gathered with torch.index_select and built again with bsi_from_values (the existence bits
    carried through) or index_from_keys (n_values as keys_at_rows derives it; a row that no column has cannot be an equality
    index's row: ValueError).  Returns the same kind of tuple, of len(order) rows."""
    import torch

    if len(index) not in (3, 5):
        raise ValueError("index is an index_from_keys result or a bsi_from_values result")
    n_rows = int(n_rows)
    if order.dtype != torch.int64 or order.dim() != 1 or order.device != index[0].device:
        raise ValueError("order: a one-dimensional int64 tensor on the index's device")
    if order.numel():
        lo, hi = (int(v) for v in torch.aminmax(order))
        if lo < 0 or hi >= n_rows:
            raise ValueError(f"order outside [0, {n_rows})")
    if len(index) == 5:
        values, have = values_of_column(wah, index, 0, n_rows)
        exists = None if have is None else torch.index_select(have, 0, order)
        return bsi_from_values(wah, torch.index_select(values, 0, order), index[3], exists=exists)
    keys = torch.index_select(keys_of_column(wah, index, 0, n_rows), 0, order)
    if keys.numel() and int(keys.min()) < 0:
        raise ValueError("a row that no column of the index has")
    n_values = (int(index[1].numel()) - 1) // (index[2] // SEGMENT_WORDS)
    return index_from_keys(wah, keys, n_values)


def select_values(wah, predicates, n_words_per_column, attributes, first=0, limit=None):
    """`SELECT a, b ... WHERE <conjunction> LIMIT limit OFFSET first` without decoding a bitmap: select_rows (predicates as for
    filter_columns), then one fetch per attribute over the rows it returned.  attributes: a list whose entries are what
    bsi_from_values returned (fetched by values_at_rows: a (values, have) pair) or what index_from_keys returned (keys_at_rows:
    a tensor of keys), all of the predicates' column length.  Returns (rows, [one result per attribute], matching rows)."""
    rows, matching = select_rows(wah, predicates, n_words_per_column, first=first, limit=limit)
    fetched = []
    for attribute in attributes:
        if attribute[2] != n_words_per_column:
            raise ValueError("an attribute of another column length")
        fetched.append(values_at_rows(wah, attribute, rows) if len(attribute) == 5 else keys_at_rows(wah, attribute, rows))
    return rows, fetched, matching


def _index_columns(seg_offsets, n_words_per_column):
    """The columns of a column-matrix index: its entries but the last one, over the segments of one column."""
    n = int(n_words_per_column)
    if n % SEGMENT_WORDS or n <= 0:
        raise ValueError("columns of a column matrix are a multiple of 992 words long")
    return (int(seg_offsets.numel()) - 1) // (n // SEGMENT_WORDS)


def splice_columns(wah, parts, n_words_per_column=None, **reuse):
    """Row ranges of column matrices concatenated into a new column matrix in one call that decodes no bitmap
    (wah_splice_indexed_device): parts is a list of ((stream, seg_offsets, n_words_per_column), first_row, n_rows), each naming
    rows [first_row, first_row + n_rows) of ALL columns of a compress_column_matrix / index_from_keys / bsi_from_values result;
    the parts have equal column counts and may differ in column length.  Column c of the result holds the parts' rows of their
    column c one after the other, and zeros behind them.  n_words_per_column defaults to the rows rounded up to a multiple of
    992 words.  reuse: source_words / scratch / out / out_offsets / check of api.splice_device (check=False returns the whole
    output buffer).  Returns (stream, seg_offsets, n_words_per_column), which go in as the arguments of the same names of
    column_operand_table and everything built on it."""
    import torch

    if not parts:
        raise ValueError("at least one part")
    pieces, tables, counts, rows = [], [], set(), 0
    for (stream, seg_offsets, n), first_row, n_rows in parts:
        first_row, n_rows = int(first_row), int(n_rows)
        if first_row < 0 or n_rows < 0 or first_row + n_rows > 32 * int(n):
            raise ValueError("a part's rows lie inside its columns")
        k = _index_columns(seg_offsets, n)
        counts.add(k)
        pieces.append((int(n), first_row, n_rows))
        tables.append(column_operand_table(stream, seg_offsets, n, torch.arange(max(k, 1), dtype=torch.int64, device=stream.device)))
        rows += n_rows
    if len(counts) != 1 or min(counts) < 1:
        raise ValueError("the parts have one column count, at least 1")
    if n_words_per_column is None:
        n_words_per_column = max(-(-((rows + 31) // 32) // SEGMENT_WORDS), 1) * SEGMENT_WORDS
    n_out = int(n_words_per_column)
    if n_out % SEGMENT_WORDS or n_out <= 0 or 32 * n_out < rows:
        raise ValueError("columns are a multiple of 992 words long and hold every row")
    check = reuse.pop("check", True)
    table = torch.cat(tables)
    got = wah.splice_device(wah.splice_pieces(pieces, table.device), table, counts.pop(), n_out, check=check, **reuse)
    if not check:
        return got[0], got[2], n_out
    return got[0], got[1], n_out


def _same_kind(index, batch):
    """What append_rows asks of its two indexes; returns the tail of the result's tuple."""
    if len(index) not in (3, 5) or len(index) != len(batch):
        raise ValueError("index and batch are both index_from_keys results or both bsi_from_values results")
    if _index_columns(index[1], index[2]) != _index_columns(batch[1], batch[2]):
        raise ValueError("index and batch differ in their column count")
    if tuple(index[3:]) != tuple(batch[3:]):
        raise ValueError("index and batch differ in n_bits or has_exists")
    return tuple(index[3:])


def append_rows(wah, index, rows, batch, batch_rows):
    """INSERT of a batch in one call: the first `rows` rows of `index` followed by the first batch_rows rows of `batch`, column by
    column (splice_columns).  index and batch are both the 3-tuple of index_from_keys or both the 5-tuple of bsi_from_values (or
    results of this function and slice_rows); ValueError when they differ in kind, in their column count, or in n_bits /
    has_exists.  Returns the same kind of tuple, its column length the rows rounded up to a multiple of 992 words; it goes into
    every call that takes the inputs."""
    tail = _same_kind(index, batch)
    return splice_columns(wah, [(tuple(index[:3]), 0, rows), (tuple(batch[:3]), 0, batch_rows)]) + tail


def slice_rows(wah, index, first, n_rows):
    """Rows [first, first + n_rows) of every column of an index as an index of its own (splice_columns with one part): a
    partition, the newest day, one GPU's share of the rows.  index: the 3-tuple of index_from_keys or the 5-tuple of
    bsi_from_values; returns the same kind of tuple, row `first` of the input being row 0 of the result."""
    if len(index) not in (3, 5):
        raise ValueError("index is an index_from_keys result or a bsi_from_values result")
    return splice_columns(wah, [(tuple(index[:3]), first, n_rows)]) + tuple(index[3:])


def _compact_rows(wah, index, mask, n_rows, n_rows_out, delete, reuse):
    """keep_rows / delete_rows: the index's columns through api.compact_device, the result sized by n_rows_out or, when that is
    None, by the count read back."""
    import torch

    if len(index) not in (3, 5):
        raise ValueError("index is an index_from_keys result or a bsi_from_values result")
    stream, seg_offsets, n = index[:3]
    k = _index_columns(seg_offsets, n)
    n_rows = int(n_rows)
    if k < 1 or n_rows < 0 or n_rows > 32 * int(n):
        raise ValueError("an index of at least one column, and rows that lie inside its columns")
    if len(mask) != 2:
        raise ValueError("mask is a (stream, seg_offsets) pair")
    bound = n_rows if n_rows_out is None else int(n_rows_out)
    if bound < 0:
        raise ValueError("n_rows_out is not negative")
    n_out = max(-(-((bound + 31) // 32) // SEGMENT_WORDS), 1) * SEGMENT_WORDS
    check = reuse.pop("check", True)
    if n_rows_out is None and not check:
        raise ValueError("check=False needs n_rows_out: the exact size comes from a count that is read back")
    table = column_operand_table(stream, seg_offsets, n, torch.arange(k, dtype=torch.int64, device=stream.device))
    got = wah.compact_device(tuple(mask), table, n, n_rows, n_out, delete=delete, check=check, **reuse)
    result, rows = (got[0], got[-2], n_out), got[-1]
    if n_rows_out is None:
        exact = max(-(-int(rows.item()) // (31 * 1024)), 1) * SEGMENT_WORDS
        if exact < n_out:  # the segments behind the last selected row are cut off: a window of the result's first rows
            result = splice_columns(wah, [(result, 0, 32 * exact)], n_words_per_column=exact)
    return result + tuple(index[3:]), rows


def keep_rows(wah, index, mask, n_rows, n_rows_out=None, **reuse):
    """`CREATE TABLE s AS SELECT * FROM t WHERE ...`, a sample, the rows a first filter kept: of the first n_rows rows of every
    column of `index`, those whose bit is set in `mask`, moved together in their order, in one call that decodes no bitmap
    (wah_compact_indexed_device).  index: the 3-tuple of index_from_keys or the 5-tuple of bsi_from_values, or a result of
    append_rows / slice_rows / keep_rows / delete_rows -- the existence slice of a bit-sliced index is compacted like any other
    column.  mask: a (stream, seg_offsets) pair over the index's column length, as filter_columns, range_column and
    compare_columns return it (the stream may be a whole output buffer of a call that was only enqueued: its index bounds what is
    read); what it holds at or behind n_rows selects nothing.  Returns (index of the same kind, rows): row i of the result is the
    i-th selected row, the rows behind them are empty, and rows is a one-element int64 device tensor, the number of selected rows.
    n_rows_out: an upper bound on that number (n_rows itself always suffices; more selected rows than 32 * the column length it
    gives are refused, WAH_ERR_STREAM) -- the result's column length is the bound rounded up to a multiple of 992 words and
    nothing is read back.  n_rows_out=None: the result is sized exactly, to max(1, ceil(rows / 31744)) segments per column; for
    that the 8-byte count is read back once, which SYNCHRONISES the stream.  reuse: source_words / scratch / out / out_offsets /
    out_rows / check of api.compact_device (check=False, which needs n_rows_out, returns the whole output buffer as the stream)."""
    return _compact_rows(wah, index, mask, n_rows, n_rows_out, False, reuse)


def delete_rows(wah, index, mask, n_rows, n_rows_out=None, **reuse):
    """`DELETE FROM t WHERE ...`, the drop of tomb-stoned rows: keep_rows with the mask complemented -- of the first n_rows rows,
    those whose bit in `mask` is CLEAR survive (WAH_COMPACT_DELETE).  Arguments, result and the synchronisation of
    n_rows_out=None as keep_rows."""
    return _compact_rows(wah, index, mask, n_rows, n_rows_out, True, reuse)


def _update_table(entries, n, dev):
    """One side of an update call: entries holds per output column the constant 0 or 1 or (index, column) -- column `column` of
    the column matrix index[:3].  The [len(entries), 3] table, constants as rows (0, bit, 0), the others through
    column_operand_table, one call per index."""
    import torch

    table = torch.tensor([(0, e, 0) if isinstance(e, int) else (0, 0, 0) for e in entries], dtype=torch.int64, device=dev)
    sources = {}
    for j, e in enumerate(entries):
        if not isinstance(e, int):
            index, column = e
            sources.setdefault(id(index), (index, [], []))
            sources[id(index)][1].append(j)
            sources[id(index)][2].append(column)
    for index, rows, columns in sources.values():
        if int(index[2]) != n or index[0].device != dev:
            raise ValueError("every index has the same column length and lies on the mask's device")
        part = column_operand_table(index[0], index[1], n, columns)
        table.index_copy_(0, torch.tensor(rows, dtype=torch.int64, device=dev), part)
    return table


def _update_columns(wah, mask, n, n_rows, else_entries, then_entries, reuse):
    """The front ends of api.update_device: the two sides as _update_table takes them; returns (stream, seg_offsets, n), with
    check=False the whole output buffer as the stream."""
    n, n_rows = int(n), int(n_rows)
    if len(mask) != 2:
        raise ValueError("mask is a (stream, seg_offsets) pair")
    if n_rows < 0 or n_rows > 32 * n:
        raise ValueError("rows that lie inside the columns")
    dev = mask[0].device
    got = wah.update_device(tuple(mask), _update_table(else_entries, n, dev), _update_table(then_entries, n, dev), n, n_rows, **reuse)
    return got[0], got[-1], n


def _whole_index(index):
    """(index, column) for every column of an index_from_keys or bsi_from_values result."""
    if len(index) not in (3, 5):
        raise ValueError("index is an index_from_keys result or a bsi_from_values result")
    k = _index_columns(index[1], index[2])
    if k < 1:
        raise ValueError("an index of at least one column")
    return [(index, c) for c in range(k)]


def update_rows(wah, index, mask, n_rows, source, **reuse):
    """`UPDATE t SET (*) = s.* FROM s WHERE ...`, the MERGE of a corrected batch into the rows it corrects: of the first n_rows
    rows of every column of `index`, those whose bit is set in `mask` take `source`'s row of the SAME number, all other rows keep
    index's, in one call that decodes no bitmap (wah_update_indexed_device).  index and source are both the 3-tuple of
    index_from_keys or both the 5-tuple of bsi_from_values (or results of append_rows / slice_rows / keep_rows / this function),
    of one kind, one column count and one column length.  mask: a (stream, seg_offsets) pair over that column length, as
    filter_columns, range_column and compare_columns return it (the stream may be the whole output buffer of a call that was only
    enqueued); what it holds at or behind n_rows selects nothing.  Returns the same kind of tuple as `index`, a NEW index that goes
    into every call that takes one.  reuse: mask_words / source_words / scratch / out / out_offsets / check of api.update_device
    (check=False returns the whole output buffer as the stream)."""
    tail = _same_kind(index, source)
    if int(index[2]) != int(source[2]):
        raise ValueError("index and source differ in their column length")
    return _update_columns(wah, mask, index[2], n_rows, _whole_index(index), _whole_index(source), reuse) + tail


def set_values_where(wah, bsi, mask, n_rows, value, **reuse):
    """`UPDATE t SET x = value WHERE ...` on a bit-sliced attribute in one call (wah_update_indexed_device): the rows below n_rows
    that `mask` selects hold `value` afterwards, all others what they held.  bsi: what bsi_from_values returned; value: an int in
    [0, 2^n_bits) -- the new slices are CONSTANTS, slice i bit n_bits - 1 - i of the value, the existence slice 1, and nothing is
    read for them -- or None, which writes NULL: every slice and the existence slice 0 (ValueError for an attribute without an
    existence slice).  mask, reuse and result as update_rows."""
    stream, seg_offsets, n, n_bits, has_exists = bsi
    if value is None:
        if not has_exists:
            raise ValueError("NULL needs an existence slice")
        bits = [0] * (n_bits + 1)
    else:
        value = int(value)
        if value < 0 or value >= 1 << n_bits:
            raise ValueError(f"value outside [0, 2^{n_bits})")
        bits = [(value >> (n_bits - 1 - i)) & 1 for i in range(n_bits)] + ([1] if has_exists else [])
    return _update_columns(wah, mask, n, n_rows, _whole_index(bsi), bits, reuse) + (n_bits, has_exists)


def set_keys_where(wah, index, mask, n_rows, key, **reuse):
    """`UPDATE t SET city = key WHERE ...` on an equality-encoded index in one call: in the rows below n_rows that `mask` selects
    column `key` is set and every other column cleared -- constants, for which nothing is read --, so a row stays in exactly one
    column.  index: what index_from_keys returned; mask, reuse and result as update_rows."""
    if len(index) != 3:
        raise ValueError("index is an index_from_keys result")
    columns = _whole_index(index)
    key = int(key)
    if key < 0 or key >= len(columns):
        raise ValueError("key names a column of the index")
    return _update_columns(wah, mask, index[2], n_rows, columns, [1 if c == key else 0 for c in range(len(columns))], reuse)


def choose_columns(wah, mask, bsi_then, bsi_else, n_rows, n_bits=None, **reuse):
    """`CASE WHEN mask THEN a ELSE b END` between two bit-sliced attributes of one column length in one call
    (wah_update_indexed_device): the rows below n_rows that `mask` selects hold bsi_then's value, all others bsi_else's.  The
    widths may differ: n_bits defaults to the wider and may not be narrower than either, the high slices an attribute lacks are
    the constant 0.  If either attribute has an existence slice the result has one; an attribute without one has a value in every
    row, the constant 1 -- in every POSITION of its columns: where bsi_else is the one without, the result's existence slice is
    set behind n_rows as well.  mask and reuse as update_rows.  Returns a bsi_from_values tuple."""
    _, _, n, kt, has_t = bsi_then
    _, _, n_e, ke, has_e = bsi_else
    if n != n_e:
        raise ValueError("the two attributes have different column lengths")
    n_bits = max(kt, ke) if n_bits is None else int(n_bits)
    if n_bits < max(kt, ke):
        raise ValueError("n_bits is not narrower than either attribute")
    has_exists = bool(has_t or has_e)

    def side(bsi, width, has):
        slices = [(bsi, width - n_bits + i) if width - n_bits + i >= 0 else 0 for i in range(n_bits)]
        return slices + ([(bsi, width) if has else 1] if has_exists else [])

    return _update_columns(wah, mask, n, n_rows, side(bsi_else, ke, has_e), side(bsi_then, kt, has_t), reuse) + (n_bits, has_exists)


def _extreme_columns(wah, op, bsi_a, bsi_b, n_rows):
    if bsi_a[4] or bsi_b[4]:
        raise ValueError("attributes without an existence slice only")
    out, _, out_offsets = compare_columns(wah, bsi_a, op, bsi_b, check=False)
    return choose_columns(wah, (out, out_offsets), bsi_a, bsi_b, n_rows)


def greatest_columns(wah, bsi_a, bsi_b, n_rows):
    """`GREATEST(a, b)` row by row between two bit-sliced attributes without existence slices (ValueError otherwise):
    compare_columns(a >= b), only enqueued, then choose_columns under its result -- two calls, nothing decoded, and nothing read
    back before the second one's status.  Returns a bsi_from_values tuple of the wider width."""
    return _extreme_columns(wah, ">=", bsi_a, bsi_b, n_rows)


def least_columns(wah, bsi_a, bsi_b, n_rows):
    """`LEAST(a, b)` row by row: greatest_columns under a <= b."""
    return _extreme_columns(wah, "<=", bsi_a, bsi_b, n_rows)


def compress_column_ranges(compressor, flat, lengths, wait=True):
    """Columns of DIFFERENT lengths (each a multiple of 992 words) stored back to back in `flat`: still one launch.
    Returns (stream, column_offsets) like compress_column_matrix: column c is stream[column_offsets[c] :
    column_offsets[c + 1]], bit-identical to compressing it alone (F4: a fill never crosses a 992-word segment)."""
    import torch

    if any(n % SEGMENT_WORDS for n in lengths) or sum(lengths) != flat.numel() or not flat.is_contiguous():
        raise ValueError("column lengths must be multiples of 992 words and add up to the buffer")
    if compressor.seg_offsets is None:
        raise ValueError("needs DeviceCompressor(..., indexed=True)")
    compressor.run(flat)
    if not wait:
        return None, None
    stream = compressor.result()
    first_segment = [0]
    for n in lengths:
        first_segment.append(first_segment[-1] + n // SEGMENT_WORDS)
    return stream, compressor.seg_offsets[torch.tensor(first_segment, device=compressor.seg_offsets.device)]


def compress_shards_multi_device(wah, shards):
    """Column shards over several GPUs by ONE call of the C ABI (include/wah.h: wah_compress_columns_multi_device): `shards` =
    list of (matrix, compressor) with matrix a contiguous [columns, n_words] tensor on the shard's device and compressor a
    DeviceCompressor(matrix.numel(), device=that device, indexed=True).  One host thread per shard inside the library, each on
    its own device and stream; nothing is exchanged.  Returns [(stream, column_offsets)] like compress_column_matrix."""
    import ctypes

    class Shard(ctypes.Structure):
        _fields_ = [("device", ctypes.c_int), ("n_columns", ctypes.c_uint64), ("d_in", ctypes.c_void_p), ("d_out", ctypes.c_void_p),
                    ("out_capacity_words", ctypes.c_uint64), ("d_out_words", ctypes.c_void_p), ("d_segment_offsets", ctypes.c_void_p),
                    ("d_workspace", ctypes.c_void_p), ("workspace_bytes", ctypes.c_size_t)]

    if not shards:
        return []
    n = shards[0][0].shape[1]
    arr = (Shard * len(shards))()
    for a, (matrix, comp) in zip(arr, shards):
        if matrix.shape[1] != n or n % SEGMENT_WORDS or not matrix.is_contiguous() or comp.seg_offsets is None:
            raise ValueError("shards need contiguous [columns, n_words] matrices of one column length (a multiple of 992) and indexed compressors")
        a.device = matrix.device.index or 0
        a.n_columns = matrix.shape[0]
        a.d_in, a.d_out, a.out_capacity_words = matrix.data_ptr(), comp.out.data_ptr(), comp.capacity
        a.d_out_words, a.d_segment_offsets = comp.count.data_ptr(), comp.seg_offsets.data_ptr()
        a.d_workspace, a.workspace_bytes = comp.workspace.data_ptr(), comp.ws_bytes
    import torch

    for matrix, _ in shards:  # (the call's streams are its own: what other streams still write into the inputs must be complete)
        torch.cuda.synchronize(matrix.device)
    status = (ctypes.c_int * len(shards))()
    rc = wah.lib().wah_compress_columns_multi_device(len(shards), ctypes.cast(arr, ctypes.c_void_p), n, ctypes.cast(status, ctypes.c_void_p))
    if rc != 0:
        raise wah.WahError(f"wah_compress_columns_multi_device: {rc} (per shard: {list(status)})")
    segs = n // SEGMENT_WORDS
    return [(comp.out[: int(comp.count.item())], comp.seg_offsets[:: segs][: matrix.shape[0] + 1]) for matrix, comp in shards]


def compress_columns(compressor, columns):
    """Enqueue one compress pass per column on the current stream; returns the list of compressed sizes
    (device tensors, read them after synchronising).  The compressor's output buffer is reused, so callers
    that need the words copy them out between columns."""
    sizes = []
    for col in columns:
        compressor.run(col)
        sizes.append(compressor.count.clone())
    return sizes


def aggregate_throughput(bytes_per_rank, seconds_per_rank):
    """Whole-job rate: all bytes / the slowest rank's time (what bench.py reports for N > 1)."""
    return sum(bytes_per_rank) / max(seconds_per_rank)

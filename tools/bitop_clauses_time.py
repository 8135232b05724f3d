"""One call over a conjunction of clauses (wah_bitop_clauses_indexed_device) against the only way to answer the same query
without it: a wah_bitop_list_indexed_device("or") call per clause, each of which leaves a compressed intermediate with its index,
then the AND of the clause results by wah_bitop_many_indexed_device (up to eight; the list call with "and" beyond) and, where
clauses are negated, one list call with "andnot" that has the AND in first place -- on the same operands, in the same process.
Queries of 2, 4 and 8 clauses with 1, 16 and 64 operands per clause, one query with two of four clauses negated, for three kinds
of 32 MiB column (tools/bitop_list_time.py: the same matrices):
  random  -- a 256-bin equality index over uniformly random keys;
  blocks  -- the same over keys sorted inside blocks of 2^20 rows;
  mixed   -- column_spec()'s columns (sparse / clustered / dense in turn).
Clause i takes the columns from i * max(1, m / 8) on, m of them, so the clauses of a query overlap: on an equality index their AND
is the bins all of them name (one-operand clauses name different bins: an empty result); the negated clauses of the negated row
lie behind the positive ones.  The chain is timed twice: with every intermediate length read back to the host, so that the
library can choose its run-merge route for the AND (a host round trip per clause), and with capacities instead of lengths.  Every
way is timed REPS times in turn (each time the mean over five calls between two events); min and max are printed -- the spread a
difference has to exceed -- and all ways must give the same words and index.  Beside the times: the algorithmic bytes, 4 x (the
operands' words + the result's words) + 8 x n_words for the one decoded intermediate, and the fraction of 8 TB/s they give over
the one call's best time.  One-clause queries are timed against the list call itself on the same table.
usage: python tools/bitop_clauses_time.py [random blocks mixed]"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
SEGS = 8457
N = 992 * SEGS  # 8 389 344 words: 32 MiB and a bit
BINS = 256
DEV = "cuda:0"
REPS = 5


def timed(run, reps=5):
    run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        run()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def equality_matrix(keys):
    """[BINS, N] int32: row v is the bitmap of keys == v, bit k of the LSB-first stream = row k."""
    m = torch.empty((BINS, N), dtype=torch.int32, device=DEV)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=DEV)
    for v in range(BINS):
        bits = (keys == v).view(N, 4, 8).to(torch.uint8)
        m[v] = (bits * weights).sum(-1).to(torch.uint8).view(torch.int32).view(N)
    return m


def make_matrix(kind):
    if kind == "mixed":
        return wah.columns.make_column_matrix(wah, [wah.columns.column_spec(c, N) for c in range(BINS)], DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(1337)
    keys = torch.randint(0, BINS, (N * 32,), dtype=torch.int16, device=DEV, generator=g)
    if kind == "blocks":
        keys = torch.cat([part.sort().values for part in keys.split(1 << 20)])
    return equality_matrix(keys)


def columns_of(matrix):
    """Every column as a stream and an index of its own."""
    comp = wah.DeviceCompressor(matrix.numel(), indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, matrix)
    starts = comp.seg_offsets[::SEGS].cpu().tolist()
    return [(stream[starts[c]: starts[c + 1]].clone(), (comp.seg_offsets[c * SEGS: (c + 1) * SEGS + 1] - starts[c]).clone()) for c in range(BINS)]


cap = wah.max_compressed_words(N)
n_seg = (cap + 1023) // 1024
scratch = torch.empty(int(lib.wah_bitop_indexed_scratch_bytes(N)), dtype=torch.uint8, device=DEV)
# the chain's intermediates: one per clause, the AND of the positive ones, the result
mid = [(torch.empty(cap, dtype=torch.int32, device=DEV), torch.zeros(n_seg + 1, dtype=torch.int64, device=DEV)) for _ in range(10)]
sp = torch.cuda.current_stream().cuda_stream


def chain(clauses, tables, andnot_table, read_back):
    """The parent's way; returns (out, count tensor, out_offsets, calls).  The list calls' tables are built beforehand, as the one
    call's are (a table's stream_words is only a bound: the intermediates' capacity serves); read_back: the 8-operand call
    sees the clause results' lengths."""
    results, calls = [], 0
    for i, (table, (_, negate)) in enumerate(zip(tables, clauses)):
        o, c, oo = wah.bitop_list_indexed_device("or", table, N, scratch=scratch, out=mid[i][0], out_offsets=mid[i][1], check=False)
        calls += 1
        results.append(((o[: int(c.item())] if read_back and not negate else o, oo), c, negate))
    pos = [r for r in results if not r[2]]
    (o, oo), c = pos[0][0], pos[0][1]
    if len(pos) > 8:
        o, c, oo = wah.bitop_list_indexed_device("and", [r[0] for r in pos], N, scratch=scratch, out=mid[-2][0], out_offsets=mid[-2][1], check=False)
        calls += 1
    elif len(pos) > 1:
        o, c, oo = wah.bitop_many_indexed_device("and", [r[0] for r in pos], N, scratch=scratch, out=mid[-2][0], out_offsets=mid[-2][1], check=False)
        calls += 1
    if andnot_table is not None:
        o, c, oo = wah.bitop_list_indexed_device("andnot", andnot_table, N, scratch=scratch, out=mid[-1][0], out_offsets=mid[-1][1], check=False)
        calls += 1
    return o, c, oo, calls


def spread(ts):
    return f"{min(ts):7.3f} .. {max(ts):7.3f}"


def row(kind, ops, n_clauses, m, negated=()):
    stride = max(1, m // 8)
    n_pos = n_clauses - len(negated)
    clauses, p, q = [], 0, 0
    for i in range(n_clauses):
        if i in negated:  # the negated clauses name columns behind the positive ones'
            start, q = (n_pos - 1) * stride + m + q * m, q + 1
        else:
            start, p = p * stride, p + 1
        clauses.append(([ops[(start + j) % BINS] for j in range(m)], i in negated))
    table, ends = wah.bitop_clause_table(clauses)
    tables = [wah.bitop_operand_table(c) for c, _ in clauses]
    andnot_table = None
    if negated:  # the AND of the positive clauses (or the one positive clause's result) first, the negated clauses' results behind it
        pos_at = -2 if n_pos > 1 else [i for i in range(n_clauses) if i not in negated][0]
        andnot_table = wah.bitop_operand_table([mid[pos_at]] + [mid[i] for i in sorted(negated)])
    res = torch.empty(cap, dtype=torch.int32, device=DEV)
    res_offs = torch.zeros(n_seg + 1, dtype=torch.int64, device=DEV)

    def one():
        return wah.bitop_clauses_indexed_device((table, ends), N, scratch=scratch, out=res, out_offsets=res_offs, check=False)

    def listed():
        return wah.bitop_list_indexed_device("or", table, N, scratch=scratch, out=mid[0][0], out_offsets=mid[0][1], check=False)

    ways = {"one call": one}
    if n_clauses == 1:
        ways["list call"] = listed
    else:
        ways["chain, lengths read back"] = lambda: chain(clauses, tables, andnot_table, True)
        ways["chain, capacities"] = lambda: chain(clauses, tables, andnot_table, False)
    times = {name: [] for name in ways}
    for _ in range(REPS):  # the ways in turn
        for name, run in ways.items():
            times[name].append(timed(run))
            assert lib.wah_bitop_indexed_status(scratch.data_ptr(), N, sp) == 0, name
    _, count, _ = one()
    torch.cuda.synchronize()
    words = int(count.item())
    calls = 1
    for name in list(ways)[1:]:
        got = ways[name]()
        o, c, oo = got[:3]
        calls = got[3] if len(got) > 3 else 1
        torch.cuda.synchronize()
        assert words == int(c.item()) and torch.equal(res[:words], o[:words]) and torch.equal(res_offs, oo), (name, "RESULTS DIFFER")
    op_words = sum(int(s.numel()) for c, _ in clauses for s, _ in c)
    nbytes = 4 * (op_words + words) + 8 * N
    t_one = times["one call"]
    others = {name: ts for name, ts in times.items() if name != "one call"}
    if n_clauses > 1:
        verdict = "faster than both" if max(t_one) < min(min(ts) for ts in others.values()) else "NOT faster by more than the spread"
    else:
        ts = others["list call"]
        verdict = "within the list call's spread" if min(t_one) <= max(ts) else f"slower than the list call by {min(t_one) - max(ts):.3f} ms beyond its spread"
    flags = f" ({len(negated)} negated)" if negated else ""
    print(f"{kind:6s} {n_clauses} clauses{flags} x {m:2d} operands: one call {spread(t_one)} ms   " +
          "   ".join(f"{name}{f' of {calls} calls' if name.startswith('chain') else ''} {spread(ts)} ms" for name, ts in others.items()) +
          f"   {op_words / (n_clauses * m) / n_seg:6.1f} words per operand and segment, result {words} words, "
          f"{nbytes / 1e6:8.1f} MB -> {nbytes / (min(t_one) * 1e-3) / 8e12:.3f} of 8 TB/s   {verdict}", flush=True)


print(f"{lib.wah_version().decode()}  columns of {N} words ({N * 4 / 2**20:.1f} MiB), {BINS} of them per kind; min .. max over {REPS} repetitions "
      f"of five calls each", flush=True)
for kind in sys.argv[1:] or ["random", "blocks", "mixed"]:
    matrix = make_matrix(kind)
    ops = columns_of(matrix)
    del matrix
    torch.cuda.empty_cache()
    for m in (1, 16, 64):
        row(kind, ops, 1, m)
    for n_clauses in (2, 4, 8):
        for m in (1, 16, 64):
            row(kind, ops, n_clauses, m)
    row(kind, ops, 4, 16, negated=(2, 3))
    del ops
    torch.cuda.empty_cache()

"""Reading a whole attribute back out of the index: columns.values_of_column / keys_of_column (one wah_values_indexed_device call)
against the two roads there were before it --
  torch     columns._values_of_column_torch: every slice decoded into the matrix [n_slices, n_words], the values assembled with
            torch shifts and ORs; for an equality index the same thing column by column (decode, unpack, torch.where), below;
  list      columns.values_at_rows / keys_at_rows with torch.arange as the list (wah_fetch_indexed_device, which walks a segment
            once per 64 listed rows).
One attribute of 1024 segments (32 505 856 rows): bit-sliced at 16, 32, 33 and 63 bits with an existence bitmap, values uniformly
random and clustered (256 distinct values, constant over runs of some thousand rows: every slice is mostly fills); an equality
index of 64 and of 4096 columns.  The three roads in one process, in turn, REPS times after one warm-up each, device events around
one call; median (min .. max).  The roads must agree.  Beside the one call's time: the bytes it moves (the table's stream words in,
8 bytes per row out) over that time, and the copy ceiling measured as bench.py --full measures it (wah_copy_device, read + write).
"one call" is the front end as a user calls it: the table is built, output and scratch are allocated, the status is read and, for
a bit-sliced attribute, the existence bit is split off the values with four torch passes over the column.  "bare call" is
api.values_device alone with table, output and scratch made before and check=False -- the kernel's own time, and the figure to
hold against the copy ceiling.
usage: python tools/values_time.py [--label TEXT] [output file]    (default: profiles/values_time.txt)"""
import argparse, importlib, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
c = wah.columns
DEV = "cuda:0"
SEGMENTS = 1024
N = SEGMENTS * 992
ROWS = 32 * N
REPS = 5

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="", help="what was measured (the commit), written into the first line")
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "values_time.txt"))
args = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(run):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    result = run()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), result


def show(ts):
    return f"{statistics.median(ts):10.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"


def copy_ceiling():
    src = torch.zeros(ROWS * 2, dtype=torch.int32, device=DEV)  # as many bytes as the call writes
    dst = torch.empty_like(src)
    for _ in range(2):
        wah.copy_device(src, dst)
    ms = timed(lambda: [wah.copy_device(src, dst) for _ in range(5)])[0]
    return 5 * 8.0 * src.numel() / (ms * 1e-3) / 1e9


def keys_torch(index):
    """keys_of_column the old way: every column decoded, unpacked and folded with torch.where, the highest column first."""
    stream, offsets, n = index
    segs = n // 992
    k = (int(offsets.numel()) - 1) // segs
    shifts = torch.arange(32, dtype=torch.int32, device=DEV)
    keys = torch.full((32 * n,), -1, dtype=torch.int64, device=DEV)
    words = torch.empty(n, dtype=torch.int32, device=DEV)
    for col in range(k - 1, -1, -1):
        wah.decompress_segments_device(stream, offsets, k * n, col * segs, segs, out=words, check=False)
        keys = torch.where(((words.view(n, 1) >> shifts) & 1).reshape(-1) != 0, col, keys)
    return keys


def same(a, b):
    if torch.is_tensor(a):
        return torch.equal(a, b)
    return torch.equal(a[0], b[0]) and (a[1] is None and b[1] is None or torch.equal(a[1], b[1]))


def case(name, stream_words, roads, table, mode):
    """roads: [(name, callable)], the one call first; table, mode: the bare call's."""
    results = [run() for _, run in roads]  # warm-up, and the roads agree
    torch.cuda.synchronize()
    for (other, _), r in zip(roads[1:], results[1:]):
        assert same(results[0], r), f"{name}: the one call and {other} DIFFER"
    del results
    ts = {road: [] for road, _ in roads}
    for _ in range(REPS):
        for road, run in roads:
            ts[road].append(timed(run)[0])
            torch.cuda.synchronize()
    one = ts[roads[0][0]]
    out = torch.empty(ROWS, dtype=torch.int64, device=DEV)
    scratch = torch.empty(int(lib.wah_values_scratch_bytes(N, table.shape[0])), dtype=torch.uint8, device=DEV)
    bare = [timed(lambda: wah.values_device(table, N, mode, out=out, scratch=scratch, check=False))[0] for _ in range(REPS + 1)][1:]
    assert lib.wah_values_status(scratch.data_ptr(), None) == 0
    del out, scratch
    moved = 4 * stream_words + 8 * ROWS
    say(f"{name}")
    for road, _ in roads:
        say(f"    {road:10s} {show(ts[road])}")
    say(f"    bare call  {show(bare)}")
    say(f"    the call moves {moved / 1e6:.1f} MB ({stream_words} words in, {ROWS} values out): {moved / (statistics.median(one) * 1e-3) / 1e9:.0f} GB/s over the one call, "
        f"{moved / (statistics.median(bare) * 1e-3) / 1e9:.0f} GB/s over the bare call ({moved / (statistics.median(bare) * 1e-3) / 1e9 / ceiling:.2f} of the copy ceiling)")
    for road, _ in roads[1:]:
        slack = max(one) - min(one)
        if statistics.median(one) <= statistics.median(ts[road]):
            say(f"    {road} / one call: {statistics.median(ts[road]) / statistics.median(one):.1f}")
        else:
            say(f"    one call SLOWER than {road} by {statistics.median(one) - statistics.median(ts[road]):.3f} ms (spread of its repetitions {slack:.3f} ms)")


def values(kind, n_bits, gen):
    if kind == "uniform":
        wide = (torch.randint(0, 1 << 32, (ROWS,), dtype=torch.int64, device=DEV, generator=gen) << 31) | torch.randint(0, 1 << 31, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
        return wide >> (63 - n_bits)
    distinct = (torch.randint(0, 1 << 32, (256,), dtype=torch.int64, device=DEV, generator=gen) << 31 | torch.randint(0, 1 << 31, (256,), dtype=torch.int64, device=DEV, generator=gen)) >> (63 - n_bits)
    runs = torch.randint(1500, 6000, (ROWS // 1500 + 2,), dtype=torch.int64, device=DEV, generator=gen)
    which = torch.randint(0, 256, (runs.numel(),), dtype=torch.int64, device=DEV, generator=gen)
    return torch.repeat_interleave(distinct[which], runs)[:ROWS].contiguous()


say(f"{lib.wah_version().decode()}  {args.label}  a whole attribute of {SEGMENTS} segments ({ROWS} rows) read back: median (min .. max) over {REPS} "
    f"repetitions, the roads in turn, device events around one call after one warm-up")
ceiling = copy_ceiling()
say(f"copy ceiling (wah_copy_device over {8 * ROWS} bytes, read + write, as bench.py --full measures it): {ceiling:.0f} GB/s")
rows_list = torch.arange(ROWS, dtype=torch.int64, device=DEV)
for kind in ("uniform", "clustered"):
    for n_bits in (16, 32, 33, 63):
        gen = torch.Generator(device=DEV).manual_seed(1337 + n_bits)
        v = values(kind, n_bits, gen)
        exists = torch.rand(ROWS, device=DEV, generator=gen) < 0.9
        bsi = c.bsi_from_values(wah, v, n_bits, n_words_per_column=N, exists=exists)
        del v, exists
        case(f"{n_bits:2d} bits + existence, {kind} values, stream {bsi[0].numel()} words", bsi[0].numel(),
             [("one call", lambda: c.values_of_column(wah, bsi)), ("torch", lambda: c._values_of_column_torch(wah, bsi)),
              ("list", lambda: c.values_at_rows(wah, bsi, rows_list))],
             c.column_operand_table(bsi[0], bsi[1], N, [n_bits] + list(range(n_bits))), wah.FETCH_BITS)
        del bsi
for n_values in (64, 4096):
    gen = torch.Generator(device=DEV).manual_seed(n_values)
    keys = torch.randint(0, n_values, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    index = c.index_from_keys(wah, keys, n_values, n_words_per_column=N)
    del keys
    case(f"equality index of {n_values} columns, uniform keys, stream {index[0].numel()} words", index[0].numel(),
         [("one call", lambda: c.keys_of_column(wah, index)), ("torch", lambda: keys_torch(index)), ("list", lambda: c.keys_at_rows(wah, index, rows_list))],
         c.column_operand_table(index[0], index[1], N, list(range(n_values))), wah.FETCH_FIRST)
    del index
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")

"""GROUP BY a bit-sliced key: api.bsi_group_by_device (one wah_bsi_group_by_indexed_device call) against the composed road there
was before it --
  composed   columns.values_of_column on the key and again on the value (8 bytes a row each), the filter decoded
             (api.decompress_segments_device) and unpacked to one bool a row, then torch.bincount and index_add_ over the rows
             it selects.
One table of 2^27 rows: a 20-slice key, uniformly random or clustered (constant over runs of some thousand rows: every slice is
mostly fills), a 32-slice uniformly random value, a filter that selects every row or about 10 %, and 256 buckets (a lookup
folds the key, key >> 12: the LDS route) or 2^20 (the key is the bucket: global atomics).  The two roads in one process, in turn,
REPS times after one warm-up each, device events around one call; median (min .. max).  The roads must agree.  "one call" is
api.bsi_group_by_device with tables, outputs and scratch made before and check=False; the composed road's tables are made before
too, its intermediates are allocated inside (they are what it costs).  Beside the times: the stream words the call reads (the
value attribute and the key twice: an item is half a segment) and the bytes the composed road writes and reads again that the
call does not (16 bytes a row of values, 1 byte a row of filter).
usage: python tools/group_by_time.py [--label TEXT] [--rows-log2 K] [output file]    (default: profiles/group_by_time.txt)"""
import argparse, importlib, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
c = wah.columns
DEV = "cuda:0"
REPS = 5
KEY_BITS, VALUE_BITS = 20, 32

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="", help="what was measured (the commit), written into the first line")
ap.add_argument("--rows-log2", type=int, default=27)
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "group_by_time.txt"))
args = ap.parse_args()
ROWS = 1 << args.rows_log2
N = -(-(ROWS // 32) // 992) * 992
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


def keys_of(kind, gen):
    if kind == "random":
        return torch.randint(0, 1 << KEY_BITS, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    runs = torch.randint(1500, 6000, (ROWS // 1500 + 2,), dtype=torch.int64, device=DEV, generator=gen)
    which = torch.randint(0, 1 << KEY_BITS, (runs.numel(),), dtype=torch.int64, device=DEV, generator=gen)
    return torch.repeat_interleave(which, runs)[:ROWS].contiguous()


def filter_of(share, gen):
    """(stream, seg_offsets) of a bitmap of N words that selects about `share` of the rows."""
    bits = torch.ones(32 * N, dtype=torch.bool, device=DEV) if share >= 1 else torch.rand(32 * N, device=DEV, generator=gen) < share
    weights = torch.ones(32, dtype=torch.int64, device=DEV) << torch.arange(32, dtype=torch.int64, device=DEV)
    words = (bits.view(N, 32).to(torch.int64) * weights).sum(1)
    words = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
    comp = wah.DeviceCompressor(N, device=DEV, indexed=True)
    comp.run(words)
    return comp.result().clone(), comp.seg_offsets.clone()


SHIFTS = torch.arange(32, dtype=torch.int32, device=DEV)


def composed(key, value, mask, lookup, n_buckets):
    keys = c.values_of_column(wah, key, 0, ROWS)[0]
    vals = c.values_of_column(wah, value, 0, ROWS)[0]
    words = wah.decompress_segments_device(mask[0], mask[1], N)[:N]
    rows = ((words.view(N, 1) >> SHIFTS) & 1).reshape(-1)[:ROWS] != 0
    buckets = (keys if lookup is None else lookup.to(torch.int64)[keys])[rows]
    counts = torch.bincount(buckets, minlength=n_buckets)
    sums = torch.zeros(n_buckets, dtype=torch.int64, device=DEV).index_add_(0, buckets, vals[rows])
    return counts, sums


say(f"{lib.wah_version().decode()}  {args.label}  GROUP BY a {KEY_BITS}-slice key with COUNT(*) and SUM of a {VALUE_BITS}-slice value over {ROWS} rows "
    f"({N} words a slice): median (min .. max) over {REPS} repetitions, the roads in turn, device events around one call after one warm-up")
gen = torch.Generator(device=DEV).manual_seed(1337)
value = c.bsi_from_values(wah, torch.randint(0, 1 << VALUE_BITS, (ROWS,), dtype=torch.int64, device=DEV, generator=gen), VALUE_BITS, n_words_per_column=N)
value_table = c.column_operand_table(value[0], value[1], N, list(range(VALUE_BITS)))
masks = {share: filter_of(share, gen) for share in (1.0, 0.1)}
scratch = torch.empty(int(lib.wah_bsi_group_by_scratch_bytes(N)), dtype=torch.uint8, device=DEV)
fold = (torch.arange(1 << KEY_BITS, dtype=torch.int64, device=DEV) >> 12).to(torch.int32)
for kind in ("random", "clustered"):
    key = c.bsi_from_values(wah, keys_of(kind, gen), KEY_BITS, n_words_per_column=N)
    key_table = c.column_operand_table(key[0], key[1], N, list(range(KEY_BITS)))
    for share, mask in masks.items():
        filters = wah.bitop_operand_table([mask])
        for n_buckets, lookup in ((256, fold), (1 << KEY_BITS, None)):
            counts = torch.empty(n_buckets + 1, dtype=torch.int64, device=DEV)
            sums = torch.empty((n_buckets + 1, 2), dtype=torch.int64, device=DEV)

            def one():
                return wah.bsi_group_by_device(key_table, N, ROWS, n_buckets, value_table=value_table, filters=filters, lookup=lookup, scratch=scratch,
                                               counts=counts, sums=sums, check=False)

            def other():
                return composed(key, value, mask, lookup, n_buckets)

            one()
            want = other()
            assert lib.wah_bsi_group_by_status(scratch.data_ptr(), None) == 0
            assert torch.equal(counts[:-1], want[0]) and torch.equal(sums[:-1, 0], want[1]) and int(counts[-1]) == 0, "the two roads DIFFER"
            selected = int(counts.sum())
            del want
            ts = {"one call": [], "composed": []}
            for _ in range(REPS):
                for road, run in (("one call", one), ("composed", other)):
                    ts[road].append(timed(run)[0])
                    torch.cuda.synchronize()
            read = 4 * (2 * (key[0].numel() + value[0].numel()) + 2 * mask[0].numel())
            say(f"{kind} keys, filter selects {100.0 * selected / ROWS:.0f} % ({selected} rows), {n_buckets} buckets{' through a lookup' if lookup is not None else ''}")
            for road in ts:
                say(f"    {road:10s} {show(ts[road])}")
            a, b = statistics.median(ts["one call"]), statistics.median(ts["composed"])
            say(f"    the call reads {read / 1e6:.1f} MB of stream words ({read / (a * 1e-3) / 1e9:.0f} GB/s); the composed road writes and reads again "
                f"{17 * ROWS / 1e6:.0f} MB that the call does not")
            say(f"    composed / one call: {b / a:.2f}" if a <= b else f"    one call SLOWER than composed: {a / b:.2f} times its time")
    del key, key_table
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")

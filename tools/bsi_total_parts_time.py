"""The TOTAL of a row's partition in every row, as a new bit-sliced attribute: columns.total_column_by (one
wah_bsi_total_parts_indexed_device call: per segment a (head, tail, has_start) record by popcounts under two masks, both scans of
the records in one workgroup, then per block of rows the partitioned running sum forward and a backward pass over its steps, and
the one-launch compressor over the result's slice matrix; check=False, so nothing is read back) against
  (a) the road there was before it: columns.values_of_column, the partitions' totals in torch -- GIVEN the starts, and the filter, as
      bool tensors on the device: the partition's number by cumsum, then the totals as differences of the values' prefix sums at
      the partitions' edges or by index_add_ into a table of one entry per partition (both timed, the verdict uses the one with
      the smaller median), and a gather back by the partition's number -- and columns.bsi_from_values (check=False) over the column of totals;
  (b) columns.cumsum_column_by at the same shape: what the second mask of the records kernel and the backward pass cost.
2^24 rows; values of 8 bits into 32 slices and of 32 bits into 56; partitions of about 2^16 rows and of about 16 rows (a start at
every row with that probability); without a filter and under a filter of one half of the rows.  The roads in one process, REPS
times in turn after a warm-up, device events around each; the median and min .. max are printed -- the spread a difference has to
exceed -- and road (a) must give the call's stream and index.  No counters and no kernel trace are taken.
usage: python tools/bsi_total_parts_time.py [output file]    (default: profiles/bsi_total_parts_time.txt)"""
import importlib, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
SHAPES = ((8, 32), (32, 56))  # (value bits, result slices)
PARTITIONS = (1 << 16, 16)    # rows per partition, about
REPS = 7

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsi_total_parts_time.txt")
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


def report(ts):
    return f"median {statistics.median(ts):8.3f} ms   {min(ts):8.3f} .. {max(ts):8.3f}   ({' '.join(f'{t:.3f}' for t in ts)})"


def verdict(new, base, what):
    ratio = statistics.median(base) / statistics.median(new)
    if max(new) < min(base):
        return f"the call faster than {what}: {ratio:.2f}x by the medians"
    if min(new) > max(base):
        return f"the call SLOWER than {what}: {1 / ratio:.2f}x by the medians"
    return f"the call and {what} within the spread ({ratio:.2f}x by the medians)"


def row(val_bits, k_out, part, filtered):
    gen = torch.Generator(device=DEV).manual_seed(9001 + val_bits + k_out + part)
    n = -(-(ROWS // 32) // 992) * 992
    values = torch.randint(0, 1 << val_bits, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    bsi = wah.columns.bsi_from_values(wah, values, val_bits, n_words_per_column=n)
    del values
    heads = torch.rand(ROWS, device=DEV, generator=gen) < 1.0 / part
    starts = wah.columns.bsi_from_values(wah, heads.to(torch.int64), 1, n_words_per_column=n)[:2]
    mask, where = None, None
    if filtered:
        mask = torch.rand(ROWS, device=DEV, generator=gen) < 0.5
        where = [wah.columns.bsi_from_values(wah, mask.to(torch.int64), 1, n_words_per_column=n)[:2]]
    scratch = torch.empty(int(lib.wah_bsi_total_parts_scratch_bytes(n, k_out, 0)), dtype=torch.uint8, device=DEV)
    running_scratch = torch.empty(int(lib.wah_bsi_cumsum_parts_scratch_bytes(n, k_out, 0)), dtype=torch.uint8, device=DEV)
    low = (1 << k_out) - 1
    n_parts = int(heads.sum().item()) + 1
    zero = torch.zeros(1, dtype=torch.int64, device=DEV)
    last = torch.full((1,), ROWS, dtype=torch.int64, device=DEV)

    def new():
        return wah.columns.total_column_by(wah, bsi, ROWS, starts, where=where, n_bits=k_out, scratch=scratch, check=False)

    def running():
        return wah.columns.cumsum_column_by(wah, bsi, ROWS, starts, where=where, n_bits=k_out, scratch=running_scratch, check=False)

    def base(by_edges=True):
        v, _ = wah.columns.values_of_column(wah, bsi, 0, ROWS)
        if mask is not None:
            v = v * mask
        number = torch.cumsum(heads, 0)  # the row's partition
        if by_edges:  # the totals as differences of the prefix sums at the partitions' edges (nonzero() waits for the host)
            front = torch.cat([zero, torch.cumsum(v, 0)])
            edges = torch.cat([zero, heads.nonzero().squeeze(1), last])
            totals = front[edges[1:]] - front[edges[:-1]]
        else:         # ... or added into a table of one entry per partition
            totals = torch.zeros(n_parts, dtype=torch.int64, device=DEV).index_add_(0, number, v)
        total = totals[number] & low
        exists = mask if mask is not None else torch.ones(ROWS, dtype=torch.bool, device=DEV)
        return wah.columns.bsi_from_values(wah, torch.where(exists, total, torch.zeros_like(total)), k_out, n_words_per_column=n, exists=exists, check=False)

    out, offsets = new()[:2]  # warm-up
    want, want_offsets = base()[:2]
    other, other_offsets = base(False)[:2]
    running()
    torch.cuda.synchronize()
    assert lib.wah_bsi_total_parts_status(scratch.data_ptr(), n, k_out, 0, None) == 0
    total = int(offsets[-1].item())
    assert int(want_offsets[-1].item()) == total and torch.equal(want[:total], out[:total]), "STREAMS DIFFER"
    assert torch.equal(want_offsets, offsets), "INDEXES DIFFER"
    assert torch.equal(other_offsets, offsets) and torch.equal(other[:total], out[:total]), "THE TWO FORMS OF (a) DIFFER"
    del out, offsets, want, want_offsets, other, other_offsets
    t_new, t_base, t_table, t_running = [], [], [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
        t_table.append(timed(lambda: base(False))[0])
        t_running.append(timed(running)[0])
    say(f"value {val_bits:2d} bits -> {k_out:2d} slices  partitions of about {part:5d} rows ({n_parts - 1} starts)  "
        f"{'filter of one half' if filtered else 'no filter'}  {ROWS} rows  result {total} words")
    say(f"    the call (total_column_by)            {report(t_new)}")
    say(f"    (a) values, totals by edges, build    {report(t_base)}")
    say(f"        ... the same by index_add_        {report(t_table)}")
    say(f"    (b) cumsum_column_by, the running sum {report(t_running)}")
    best = t_base if statistics.median(t_base) <= statistics.median(t_table) else t_table
    say(f"    {verdict(t_new, best, '(a)')}; {verdict(t_new, t_running, '(b)')}")


say(f"{lib.wah_version().decode()}  median and min .. max over {REPS} repetitions in turn after a warm-up, device events around each road")
for val_bits, k_out in SHAPES:
    for part in PARTITIONS:
        for filtered in (False, True):
            row(val_bits, k_out, part, filtered)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

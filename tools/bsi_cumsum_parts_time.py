"""The running sum PER PARTITION of a bit-sliced attribute as a new bit-sliced attribute: columns.cumsum_column_by (one
wah_bsi_cumsum_parts_indexed_device call: per segment a (has_start, tail) record by popcounts, the segmented scan of the records,
then the rows scanned 64 at a time, a step that holds a start corrected by its exclusive value at the lane's head lane, and the
one-launch compressor over the result's slice matrix; check=False, so nothing is read back) against
  (a) the road there was before it: columns.values_of_column, a segmented cumsum in torch -- GIVEN the starts, and the filter, as
      bool tensors on the device: cumsum, minus the sum in front of the row's partition, looked up in a table of one entry per
      partition by the partition's number (the faster form, which the verdict uses), or gathered from the last start at or in
      front of the row, found by cummax (timed too) -- and columns.bsi_from_values (check=False) over the scanned column;
  (b) columns.cumsum_column at the same shape: what the resets cost.
2^24 rows; values of 8 bits into 32 slices and of 32 bits into 56; partitions of about 2^16 rows and of about 16 rows (a start at
every row with that probability); without a filter and under a filter of one half of the rows.  The three roads in one process,
REPS times in turn after a warm-up, device events around each; the median and min .. max are printed -- the spread a difference has
to exceed -- and road (a) must give the call's stream and index.
usage: python tools/bsi_cumsum_parts_time.py [output file]    (default: profiles/bsi_cumsum_parts_time.txt)"""
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

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsi_cumsum_parts_time.txt")
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
    scratch = torch.empty(int(lib.wah_bsi_cumsum_parts_scratch_bytes(n, k_out, 0)), dtype=torch.uint8, device=DEV)
    plain_scratch = torch.empty(int(lib.wah_bsi_cumsum_scratch_bytes(n, k_out, 0)), dtype=torch.uint8, device=DEV)
    low = (1 << k_out) - 1
    numbers = torch.arange(ROWS, dtype=torch.int64, device=DEV)

    def new():
        return wah.columns.cumsum_column_by(wah, bsi, ROWS, starts, where=where, n_bits=k_out, scratch=scratch, check=False)

    def plain():
        return wah.columns.cumsum_column(wah, bsi, ROWS, where=where, n_bits=k_out, scratch=plain_scratch, check=False)

    def base(by_table=True):
        v, _ = wah.columns.values_of_column(wah, bsi, 0, ROWS)
        if mask is not None:
            v = v * mask
        run = torch.cumsum(v, 0)
        if by_table:  # the sum in front of every partition, looked up by the partition's number (nonzero() waits for the host)
            at = heads.nonzero().squeeze(1)
            front = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), (run - v)[at]])[torch.cumsum(heads, 0)]
        else:         # ... or gathered from the last start at or in front of a row, found by cummax
            last = torch.cummax(torch.where(heads, numbers, torch.zeros_like(numbers)), 0).values
            front = torch.where(torch.cumsum(heads, 0) > 0, (run - v)[last], torch.zeros_like(run))
        run = (run - front) & low
        exists = mask if mask is not None else torch.ones(ROWS, dtype=torch.bool, device=DEV)
        return wah.columns.bsi_from_values(wah, torch.where(exists, run, torch.zeros_like(run)), k_out, n_words_per_column=n, exists=exists, check=False)

    out, offsets = new()[:2]  # warm-up
    want, want_offsets = base()[:2]
    other, other_offsets = base(False)[:2]
    plain()
    torch.cuda.synchronize()
    assert lib.wah_bsi_cumsum_parts_status(scratch.data_ptr(), n, k_out, 0, None) == 0
    total = int(offsets[-1].item())
    assert int(want_offsets[-1].item()) == total and torch.equal(want[:total], out[:total]), "STREAMS DIFFER"
    assert torch.equal(want_offsets, offsets), "INDEXES DIFFER"
    assert torch.equal(other_offsets, offsets) and torch.equal(other[:total], out[:total]), "THE TWO FORMS OF (a) DIFFER"
    del out, offsets, want, want_offsets, other, other_offsets
    t_new, t_base, t_cummax, t_plain = [], [], [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
        t_cummax.append(timed(lambda: base(False))[0])
        t_plain.append(timed(plain)[0])
    say(f"value {val_bits:2d} bits -> {k_out:2d} slices  partitions of about {part:5d} rows ({int(heads.sum().item())} starts)  "
        f"{'filter of one half' if filtered else 'no filter'}  {ROWS} rows  result {total} words")
    say(f"    the call (cumsum_column_by)          {report(t_new)}")
    say(f"    (a) values, segmented cumsum, build  {report(t_base)}")
    say(f"        ... the same by cummax and gather {report(t_cummax)}")
    say(f"    (b) cumsum_column, no partitions     {report(t_plain)}")
    say(f"    {verdict(t_new, t_base, '(a)')}; {verdict(t_new, t_plain, '(b)')}")


say(f"{lib.wah_version().decode()}  median and min .. max over {REPS} repetitions in turn after a warm-up, device events around each road")
for val_bits, k_out in SHAPES:
    for part in PARTITIONS:
        for filtered in (False, True):
            row(val_bits, k_out, part, filtered)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

"""The running sum of a bit-sliced attribute as a new bit-sliced attribute: columns.cumsum_column (one
wah_bsi_cumsum_indexed_device call: the segments' totals by popcounts, their scan, then the value's compressed slices folded into a
word per row in LDS, scanned 64 rows at a time and transposed in registers into slice words, and the one-launch compressor over the
result's slice matrix; check=False, so nothing is read back) against the road there was before it: columns.values_of_column (one
wah_values_indexed_device call that writes 8 bytes a row), torch.cumsum, and columns.bsi_from_values (check=False) over the scanned
column.  2^24 rows; values of 8 and of 32 bits; results of 32 and of 56 slices; without a filter and under a filter of one half of
the rows, which the composed road is GIVEN as a bool tensor on the device (it has no way of its own to read one from the index).
Both roads in one process, REPS times in turn after a warm-up, device events around each; the median and min .. max are printed --
the spread a difference has to exceed -- and both roads must give the same stream and index.
usage: python tools/bsi_cumsum_time.py [output file]    (default: profiles/bsi_cumsum_time.txt)"""
import importlib, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
VAL_BITS = (8, 32)
OUT_BITS = (32, 56)
REPS = 7

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsi_cumsum_time.txt")
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


def verdict(new, base):
    ratio = statistics.median(base) / statistics.median(new)
    if max(new) < min(base):
        return f"one call faster: {ratio:.2f}x by the medians"
    if min(new) > max(base):
        return f"one call SLOWER: {1 / ratio:.2f}x by the medians"
    return f"within the spread ({ratio:.2f}x by the medians)"


def row(val_bits, k_out, filtered):
    gen = torch.Generator(device=DEV).manual_seed(9001 + val_bits + k_out)
    n = -(-(ROWS // 32) // 992) * 992
    values = torch.randint(0, 1 << val_bits, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    bsi = wah.columns.bsi_from_values(wah, values, val_bits, n_words_per_column=n)
    del values
    mask, where = None, None
    if filtered:
        mask = torch.rand(ROWS, device=DEV, generator=gen) < 0.5
        f_stream, f_offsets = wah.columns.bsi_from_values(wah, mask.to(torch.int64), 1, n_words_per_column=n)[:2]
        where = [(f_stream, f_offsets)]
    flags = 0
    scratch = torch.empty(int(lib.wah_bsi_cumsum_scratch_bytes(n, k_out, flags)), dtype=torch.uint8, device=DEV)
    low = (1 << k_out) - 1

    def new():
        return wah.columns.cumsum_column(wah, bsi, ROWS, where=where, n_bits=k_out, scratch=scratch, check=False)

    def base():
        v, _ = wah.columns.values_of_column(wah, bsi, 0, ROWS)
        if mask is not None:
            v = v * mask
        run = torch.cumsum(v, 0) & low
        exists = mask if mask is not None else torch.ones(ROWS, dtype=torch.bool, device=DEV)
        return wah.columns.bsi_from_values(wah, torch.where(exists, run, torch.zeros_like(run)), k_out, n_words_per_column=n, exists=exists, check=False)

    out, offsets = new()[:2]  # warm-up
    want, want_offsets = base()[:2]
    torch.cuda.synchronize()
    assert lib.wah_bsi_cumsum_status(scratch.data_ptr(), n, k_out, flags, None) == 0
    total = int(offsets[-1].item())
    assert int(want_offsets[-1].item()) == total and torch.equal(want[:total], out[:total]), "STREAMS DIFFER"
    assert torch.equal(want_offsets, offsets), "INDEXES DIFFER"
    del out, offsets, want, want_offsets
    t_new, t_base = [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
    say(f"value {val_bits:2d} bits  -> {k_out:2d} slices  {'filter of one half' if filtered else 'no filter         '}  {ROWS} rows  value stream {int(bsi[0].numel())} words  result {total} words")
    say(f"    one call                        {report(t_new)}")
    say(f"    values, torch.cumsum, build     {report(t_base)}")
    say(f"    {verdict(t_new, t_base)}")


say(f"{lib.wah_version().decode()}  median and min .. max over {REPS} repetitions in turn after a warm-up, device events around each road")
for val_bits in VAL_BITS:
    for k_out in OUT_BITS:
        for filtered in (False, True):
            row(val_bits, k_out, filtered)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

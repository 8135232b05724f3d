"""A bit-sliced key through a lookup table as a new bit-sliced attribute: columns.map_column (one wah_bsi_map_indexed_device call: the
key's compressed slices folded into a word per row in LDS, one table load per row, the values transposed in registers into slice
words, then the one-launch compressor over the result's slice matrix; check=False, so nothing is read back) against the road
there was before it: columns.values_of_column (one wah_values_indexed_device call that writes 8 bytes a row), lookup[values] in
torch, and columns.bsi_from_values (check=False) over the gathered column.  2^24 rows; keys of 12 and of 24 bits; lookups of 4 Ki
and of 16 Mi entries (the second does not fit an XCD's L2); results of 8 and of 32 bits; uniform keys and sorted keys.  Both roads
in one process, REPS times in turn after a warm-up, device events around each; every time and min .. max are printed -- the spread
a difference has to exceed -- and both roads must give the same stream and index.  The bytes are the LEAST each road moves,
computed from the shapes: the one call reads the key's stream and one 4-byte entry a row, writes and reads the result's slice
matrix and writes its stream; the composition also writes and reads an int64 per row twice.
usage: python tools/bsi_map_time.py [output file]    (default: profiles/bsi_map_time.txt)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
SHAPES = ((12, 1 << 12), (24, 1 << 24))  # bits of the key, entries of the lookup
OUT_BITS = (8, 32)
REPS = 5

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsi_map_time.txt")
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


def spread(ts):
    return f"{min(ts):9.3f} .. {max(ts):9.3f}"


def every(ts):
    return " ".join(f"{t:.3f}" for t in ts)


def verdict(new, base):
    if max(new) < min(base):
        return f"one call faster, {min(base) / max(new):.1f}x at the least"
    if min(new) > max(base):
        return f"one call SLOWER, {min(new) / max(base):.1f}x at the least"
    return "within the spread"


def row(key_bits, n_keys, k_out, order):
    gen = torch.Generator(device=DEV).manual_seed(7001 + key_bits + k_out)
    n = -(-(ROWS // 32) // 992) * 992
    keys = torch.randint(0, n_keys, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    if order == "sorted":
        keys = torch.sort(keys)[0]
    key = wah.columns.bsi_from_values(wah, keys, key_bits, n_words_per_column=n)
    del keys
    top = (1 << k_out) - 1 - (1 if k_out == 32 else 0)  # (2^32 - 1 is the null entry)
    lookup64 = torch.randint(0, top + 1, (n_keys,), dtype=torch.int64, device=DEV, generator=gen)
    lookup = wah.columns._lookup_tensor(lookup64, torch.device(DEV))
    scratch = torch.empty(int(lib.wah_bsi_map_scratch_bytes(n, k_out, 0)), dtype=torch.uint8, device=DEV)

    def new():
        return wah.columns.map_column(wah, key, ROWS, lookup, n_bits=k_out, scratch=scratch, check=False)

    def base():
        values, _ = wah.columns.values_of_column(wah, key, 0, ROWS)
        return wah.columns.bsi_from_values(wah, lookup64[values], k_out, n_words_per_column=n, check=False)

    out, offsets = new()[:2]  # warm-up
    want, want_offsets = base()[:2]
    torch.cuda.synchronize()
    assert lib.wah_bsi_map_status(scratch.data_ptr(), n, k_out, 0, None) == 0
    total = int(offsets[-1].item())
    assert int(want_offsets[-1].item()) == total and torch.equal(want[:total], out[:total]), "STREAMS DIFFER"
    assert torch.equal(want_offsets, offsets), "INDEXES DIFFER"
    del out, offsets, want, want_offsets
    t_new, t_base = [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
    in_bytes, matrix, column = 4 * int(key[0].numel()), 4 * k_out * n, 8 * ROWS
    new_bytes = in_bytes + 4 * ROWS + 2 * matrix + 4 * total
    base_bytes = in_bytes + 2 * column + 4 * ROWS + 2 * column + 2 * matrix + 4 * total
    say(f"key {key_bits:2d} bits  lookup {n_keys:8d} entries  -> {k_out:2d} bits  {order:7s} keys  {ROWS} rows  key stream {int(key[0].numel())} words  result {total} words")
    say(f"    one call                        {spread(t_new)} ms   ({every(t_new)})   at least {new_bytes / 1e6:8.1f} MB moved")
    say(f"    values, torch gather, build     {spread(t_base)} ms   ({every(t_base)})   at least {base_bytes / 1e6:8.1f} MB moved")
    say(f"    {verdict(t_new, t_base)}")


say(f"{lib.wah_version().decode()}  min .. max over {REPS} repetitions in turn after a warm-up, device events around each road")
for key_bits, n_keys in SHAPES:
    for k_out in OUT_BITS:
        for order in ("uniform", "sorted"):
            row(key_bits, n_keys, k_out, order)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

"""Multiplying two bit-sliced attributes row by row: columns.multiply_columns (one wah_bsi_mul_indexed_device call: the shift-and-add
sweep over the operands' compressed slices, then the one-launch compressor over the product's slice matrix; check=False, so
nothing is read back) against the road there was before it: decode both attributes' streams to their slice matrices
(DeviceDecompressor, made outside the timed part), turn the matrices into value columns with torch ops (per slice an unpack of
the words into one int64 per row, a shift and an OR), multiply the columns with torch, and build the product's index again
(columns.bsi_from_values, check=False).  2^24 rows of uniform random values, 8 x 8 -> 16, 20 x 20 -> 40 and 32 x 32 -> 63 bits,
without and with existence tensors of density 0.7; and one more row, 20 x 20 -> 40 with a multiplier that is a CONSTANT of three
set bits, which shows what the skip of a zero slice is worth.  Both roads in one process, REPS times in turn after a warm-up,
device events around each; every time and min .. max are printed -- the spread a difference has to exceed -- and both roads must
give the same stream and index.  The bytes are the LEAST each road moves, computed from the shapes; the one call's include the
sweep's working area (A's image written once and read once per slice of B that is not skipped, the accumulator read and written
by every step), which is traffic whether or not a cache holds it.
usage: python tools/bsi_mul_time.py [output file]    (default: profiles/bsi_mul_time.txt)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
SHAPES = ((8, 16), (20, 40), (32, 63))  # bits of either operand, bits of the product
CONSTANT = (1 << 17) | (1 << 9) | 1  # three set bits of twenty
REPS = 5

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsi_mul_time.txt")
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


def uniform(gen, n_bits):
    wide = (torch.randint(0, 1 << 32, (ROWS,), dtype=torch.int64, device=DEV, generator=gen) << 31) | torch.randint(0, 1 << 31, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    return wide >> (63 - n_bits)  # uniform over [0, 2^n_bits): every slice is incompressible


SHIFTS = torch.arange(32, dtype=torch.int64, device=DEV)


def unpack(words):
    """int32 words [n] -> int64 0 / 1 per row [32 n], row p at word p // 32, bit p % 32."""
    return ((words.to(torch.int64).view(-1, 1) >> SHIFTS) & 1).view(-1)


def row(n_bits, k_out, with_exists, constant=None):
    gen = torch.Generator(device=DEV).manual_seed(5151 + n_bits)
    n = -(-(ROWS // 32) // 992) * 992
    attributes = []
    for which in range(2):
        values = uniform(gen, n_bits)
        if which == 1 and constant is not None:
            values.fill_(constant)
        exists = (torch.rand(ROWS, device=DEV, generator=gen) < 0.7) if with_exists else None
        attributes.append(wah.columns.bsi_from_values(wah, values, n_bits, n_words_per_column=n, exists=exists))
        del values, exists
    a, b = attributes
    rows_in = n_bits + (1 if with_exists else 0)
    rows_out = k_out + (1 if with_exists else 0)
    decoders = [wah.DeviceDecompressor(int(x[0].numel()), rows_in * n) for x in attributes]
    table = torch.empty((2 * rows_in, 3), dtype=torch.int64, device=DEV)
    flags = (wah.BSI_EXISTS_A | wah.BSI_EXISTS_B) if with_exists else 0
    scratch = torch.empty(int(lib.wah_bsi_mul_scratch_bytes(n, n_bits, k_out, flags)), dtype=torch.uint8, device=DEV)

    def new():
        return wah.columns.multiply_columns(wah, a, b, n_bits=k_out, table=table, scratch=scratch, check=False)

    def base():
        columns, have = [], None
        for decoder, (stream, _, _, bits, _) in zip(decoders, attributes):
            decoder.run(stream)
            matrix = decoder.out[: rows_in * n].view(rows_in, n)
            v = torch.zeros(32 * n, dtype=torch.int64, device=DEV)
            for i in range(bits):
                v |= unpack(matrix[i]) << (bits - 1 - i)
            columns.append(v)
            if with_exists:
                e = unpack(matrix[bits]) != 0
                have = e if have is None else have & e
        product = (columns[0] * columns[1]) & ((1 << k_out) - 1)  # (int64 wraps mod 2^64, which 2^k_out divides)
        return wah.columns.bsi_from_values(wah, product, k_out, n_words_per_column=n, exists=have, check=False)

    out, offsets = new()[:2]  # warm-up
    want, want_offsets = base()[:2]
    torch.cuda.synchronize()
    for decoder in decoders:
        decoder.status()
    total = int(offsets[-1].item())
    assert int(want_offsets[-1].item()) == total and torch.equal(want[:total], out[:total]), "STREAMS DIFFER"
    assert torch.equal(want_offsets, offsets), "INDEXES DIFFER"
    del out, offsets, want, want_offsets
    t_new, t_base = [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
    # the least each road moves: compressed words in and out, the decoded slice matrices written and read, one int64 per row and
    # column; the one call's working area: 4 KiB per segment and slice -- A's image written, then per slice j of B that is not
    # skipped A's slices read and the accumulator's read and written (slice 0 only writes), one carry slot each, and the
    # accumulator read once behind the sweep
    ka = kb = n_bits
    segs = n // 992
    slices = ka + min(k_out, ka + kb)
    for j in range(kb):
        steps = max(min(ka, k_out - j), 0)
        if j == 0:
            slices += 2 * steps
        elif constant is None or (constant >> j) & 1:
            slices += 3 * steps
        slices += 1 if ka + j < k_out else 0
    work = 4096 * segs * slices
    in_bytes = 4 * (int(a[0].numel()) + int(b[0].numel()))
    out_matrix, in_matrices, column = 4 * rows_out * n, 2 * 4 * rows_in * n, 8 * 32 * n
    new_bytes = in_bytes + work + 2 * out_matrix + 4 * total
    base_bytes = in_bytes + 2 * in_matrices + 2 * column + 3 * column + column + 2 * out_matrix + 4 * total
    what = f"{n_bits:2d} x {n_bits:2d} -> {k_out:2d} bits" + ("" if constant is None else f"  B = {constant:#x} in every row")
    say(f"{what}  existence {'yes' if with_exists else 'no ':3s}  {ROWS} rows  slices of {n} words  stream {total} words")
    say(f"    one call                      {spread(t_new)} ms   ({every(t_new)})   at least {new_bytes / 1e6:9.1f} MB moved, {work / 1e6:.1f} of them in the working area")
    say(f"    decode, torch multiply, build {spread(t_base)} ms   ({every(t_base)})   at least {base_bytes / 1e6:9.1f} MB moved")
    say(f"    {verdict(t_new, t_base)}")


say(f"{lib.wah_version().decode()}  min .. max over {REPS} repetitions in turn after a warm-up, device events around each road; uniform random values")
for n_bits, k_out in SHAPES:
    for with_exists in (False, True):
        row(n_bits, k_out, with_exists)
row(20, 40, False, constant=CONSTANT)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

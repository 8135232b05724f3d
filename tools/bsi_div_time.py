"""Dividing two bit-sliced attributes row by row: columns.divide_columns as a caller has it -- the row table rewritten in place, one
wah_bsi_div_indexed_device call enqueued (the long-division sweep over the operands' compressed slices, then the one-launch
compressor over the quotient's slice matrix), the status read -- against the road there was before it: columns.values_of_column
for both attributes, a torch floor-divide over the two value columns (the divisor's zeros replaced by 1 and taken out of the
existence tensor: torch's own division by zero is undefined), and columns.bsi_from_values again, its status read too.  2^24 rows,
16 / 8, 32 / 16, 32 / 32 and 63 / 31 bits, without and with existence tensors of density 0.7, with uniform values of the full
width and with values of a QUARTER of their declared width, which shows what the skips of the leading zero slices of either
operand are worth.  The divisor is 0 in one row of sixteen.  Both roads in one process, REPS times in turn after a warm-up,
device events around each; every time and min .. max are printed -- the spread a difference has to exceed -- and both roads must
give the same stream and index.  The bytes are the LEAST each road moves, computed from the shapes; the one call's include the sweep's working
area (B's image written once; per step of the ka slices of A that are not skipped and per slice of B one read of B, R and T and
one write of R and T), which is traffic whether or not a cache holds it.
usage: python tools/bsi_div_time.py [output file]    (default: profiles/bsi_div_time.txt)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
SHAPES = ((16, 8), (32, 16), (32, 32), (63, 31))  # bits of the dividend, of the divisor
REPS = 5

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsi_div_time.txt")
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


def row(ka, kb, with_exists, quarter):
    gen = torch.Generator(device=DEV).manual_seed(6161 + ka)
    n = -(-(ROWS // 32) // 992) * 992
    attributes = []
    for which, bits in enumerate((ka, kb)):
        real = max(bits // 4, 1) if quarter else bits
        values = uniform(gen, real)
        if which == 1:
            values[torch.rand(ROWS, device=DEV, generator=gen) < 1.0 / 16.0] = 0
        exists = (torch.rand(ROWS, device=DEV, generator=gen) < 0.7) if with_exists else None
        attributes.append(wah.columns.bsi_from_values(wah, values, bits, n_words_per_column=n, exists=exists))
        del values, exists
    a, b = attributes
    rows_in = with_exists + 0
    table = torch.empty((ka + kb + 2 * rows_in, 3), dtype=torch.int64, device=DEV)
    flags = (wah.BSI_EXISTS_A | wah.BSI_EXISTS_B) if with_exists else 0
    scratch = torch.empty(int(lib.wah_bsi_div_scratch_bytes(n, kb, ka, flags)), dtype=torch.uint8, device=DEV)
    out = torch.empty(wah.max_compressed_words((ka + 1) * n), dtype=torch.int32, device=DEV)
    out_offsets = torch.zeros((ka + 1) * (n // 992) + 1, dtype=torch.int64, device=DEV)

    def new():
        return wah.columns.divide_columns(wah, a, b, table=table, scratch=scratch, out=out, out_offsets=out_offsets)

    def base():
        va, have_a = wah.columns.values_of_column(wah, a)
        vb, have_b = wah.columns.values_of_column(wah, b)
        have = vb != 0
        if with_exists:
            have &= have_a & have_b
        quotient = torch.div(va, torch.where(vb != 0, vb, torch.ones_like(vb)), rounding_mode="floor")
        return wah.columns.bsi_from_values(wah, quotient, ka, n_words_per_column=n, exists=have)

    got, offsets = new()[:2]  # warm-up
    got, offsets = got.clone(), offsets.clone()
    want, want_offsets = base()[:2]
    torch.cuda.synchronize()
    total = int(offsets[-1].item())
    assert int(want_offsets[-1].item()) == total and torch.equal(want[:total], got[:total]), "STREAMS DIFFER"
    assert torch.equal(want_offsets, offsets), "INDEXES DIFFER"
    del got, offsets, want, want_offsets
    t_new, t_base = [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
    # the least each road moves: compressed words in and out, the quotient's decoded slice matrix written and read, one int64 per
    # row and column; the one call's working area, 4 KiB per segment and slice: B's image written, then per step of A that is not
    # skipped and per slice of B that is not left out three reads and two writes (the first step reads B alone), and the quotient
    # slice read and written by each step
    segs = n // 992
    steps, run = (max(ka // 4, 1), max(kb // 4, 1)) if quarter else (ka, kb)
    slices = kb + steps * (run * 5 + 2) - 2 * run
    work = 4096 * segs * slices
    in_bytes = 4 * (int(a[0].numel()) + int(b[0].numel()))
    out_matrix, column = 4 * (ka + 1) * n, 8 * 32 * n
    new_bytes = in_bytes + work + 2 * out_matrix + 4 * total
    base_bytes = in_bytes + 2 * column + 3 * column + column + 2 * out_matrix + 4 * total
    what = f"{ka:2d} / {kb:2d} bits, values of {'a quarter of' if quarter else 'the whole of '} their width"
    say(f"{what}  existence {'yes' if with_exists else 'no ':3s}  {ROWS} rows  slices of {n} words  stream {total} words")
    say(f"    one call                      {spread(t_new)} ms   ({every(t_new)})   at least {new_bytes / 1e6:9.1f} MB moved, {work / 1e6:.1f} of them in the working area")
    say(f"    values, torch divide, build   {spread(t_base)} ms   ({every(t_base)})   at least {base_bytes / 1e6:9.1f} MB moved")
    say(f"    {verdict(t_new, t_base)}")


say(f"{lib.wah_version().decode()}  min .. max over {REPS} repetitions in turn after a warm-up, device events around each road; the status read in both")
for ka, kb in SHAPES:
    for with_exists in (False, True):
        for quarter in (False, True):
            row(ka, kb, with_exists, quarter)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

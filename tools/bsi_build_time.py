"""Building the bit-sliced index of a value column: columns.bsi_from_values (one wah_bsi_build_device call: the transpose kernel,
then the one-launch compressor over its slice matrix; check=False, so nothing is read back) against the way there was before it,
columns._bsi_from_values_torch (per slice a shift and mask of the whole column, a zeroed int64 tensor of one entry per row, a
multiply and a row sum, then the same compressor; it reads the values' minimum and maximum back and makes its compressor inside).
2^24 rows of uniform random values at 8, 20 and 63 bits, without and with an existence tensor of density 0.7.  Both ways in one
process, REPS times in turn after a warm-up, device events around each; every time and min .. max are printed -- the spread a
difference has to exceed -- and both ways must give the same stream and index.
usage: python tools/bsi_build_time.py [output file]    (default: profiles/bsi_build_time.txt)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
BITS = (8, 20, 63)
REPS = 5

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bsi_build_time.txt")
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


def row(n_bits, with_exists):
    gen = torch.Generator(device=DEV).manual_seed(1337 + n_bits)
    wide = (torch.randint(0, 1 << 32, (ROWS,), dtype=torch.int64, device=DEV, generator=gen) << 31) | torch.randint(0, 1 << 31, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    values = wide >> (63 - n_bits)  # uniform over [0, 2^n_bits): every slice is incompressible
    del wide
    exists = (torch.rand(ROWS, device=DEV, generator=gen) < 0.7) if with_exists else None
    n = -(-(ROWS // 32) // 992) * 992

    def new():
        return wah.columns.bsi_from_values(wah, values, n_bits, n_words_per_column=n, exists=exists, check=False)

    def base():
        return wah.columns._bsi_from_values_torch(wah, values, n_bits, n_words_per_column=n, exists=exists)

    out, offsets = new()[:2]  # warm-up
    want, want_offsets = base()[:2]
    torch.cuda.synchronize()
    total = int(offsets[-1].item())
    assert want.numel() == total and torch.equal(want, out[:total]), "STREAMS DIFFER"
    assert torch.equal(want_offsets, offsets), "INDEXES DIFFER"
    del out, offsets, want, want_offsets
    t_new, t_base = [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
    say(f"{n_bits:2d} bits  existence {'yes' if with_exists else 'no ':3s}  {ROWS} rows  slices of {n} words  stream {total} words")
    say(f"    one call   {spread(t_new)} ms   ({every(t_new)})")
    say(f"    torch ops  {spread(t_base)} ms   ({every(t_base)})")
    say(f"    {verdict(t_new, t_base)}")


say(f"{lib.wah_version().decode()}  min .. max over {REPS} repetitions in turn after a warm-up, device events around each way; uniform random values")
for n_bits in BITS:
    for with_exists in (False, True):
        row(n_bits, with_exists)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

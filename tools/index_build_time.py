"""Building the equality-encoded index of a key column: columns.index_from_keys (one stable torch.sort, one torch.bincount, one
wah_from_positions_device call; no decoded bitmap) against the only way there was before it: the decoded one-hot bit matrix
[n_values, n_words] made with torch (zeros + one index_add_ of every row's bit: the bits of a word are distinct, so adding them is
OR-ing them) and compress_column_matrix over it, the matrix's making included; the compressor and its output are made before the
clock starts.  2^24 rows of uniform random keys; 16, 256 and 4096 values (4096: a matrix of 8 GiB -- where it does not fit beside
the compressor's output that is recorded instead of a time).  Both ways in one process, REPS times in turn after a warm-up, device
events around each; min and max are printed -- the spread a difference has to exceed -- and both ways must give the same stream and
index.
usage: python tools/index_build_time.py [output file] [trace]    (default: profiles/from_positions_times.txt; `trace`: 256
values only, each way once after its warm-up -- the run to put under `rocprofv3 --kernel-trace --stats`)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
VALUES = (16, 256, 4096)
REPS = 5

args = sys.argv[1:]
trace = "trace" in args
args = [a for a in args if a != "trace"]
out_path = args[0] if args else os.path.join(ROOT, "profiles", "from_positions_times.txt")
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


def verdict(new, base):
    if max(new) < min(base):
        return f"from rows faster, {min(base) / max(new):.1f}x at the least"
    if min(new) > max(base):
        return f"from rows SLOWER, {min(new) / max(base):.1f}x at the least"
    return "within the spread"


def row(n_values):
    keys = torch.randint(0, n_values, (ROWS,), dtype=torch.int64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1337 + n_values))
    n = -(-(ROWS // 32) // 992) * 992
    matrix_bytes = 4 * n_values * n

    def new():
        return wah.columns.index_from_keys(wah, keys, n_values, check=False)

    out, offsets, n_new = new()  # warm-up
    torch.cuda.synchronize()
    assert n_new == n
    total = int(offsets[-1].item())
    free, _ = torch.cuda.mem_get_info()
    # the matrix, the compressor's output (as long at the worst) and workspace, index_add_'s index and values
    need = 2 * matrix_bytes + int(lib.wah_compress_workspace_bytes(n_values * n)) + 16 * ROWS + (1 << 30)
    if need > free:
        t_new = [timed(new)[0] for _ in range(REPS)]
        say(f"{n_values:5d} values  {ROWS} rows  columns of {n} words  stream {total} words   from rows {spread(t_new)} ms   "
            f"matrix + compress: DID NOT FIT (matrix {matrix_bytes / 2**30:.2f} GiB, {need / 2**30:.1f} GiB needed, {free / 2**30:.1f} GiB free)")
        return
    comp = wah.DeviceCompressor(n_values * n, indexed=True)
    word = torch.arange(ROWS, dtype=torch.int64, device=DEV)

    def base():
        matrix = torch.zeros(n_values * n, dtype=torch.int32, device=DEV)
        matrix.index_add_(0, keys * n + (word >> 5), (1 << (word & 31)).to(torch.int32))
        wah.columns.compress_column_matrix(comp, matrix.view(n_values, n), wait=False)

    base()  # warm-up
    want = comp.result()
    assert want.numel() == total and torch.equal(want, out[:total]), "STREAMS DIFFER"
    assert torch.equal(comp.seg_offsets, offsets), "INDEXES DIFFER"
    t_new, t_base = [], []
    for _ in range(1 if trace else REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
    say(f"{n_values:5d} values  {ROWS} rows  columns of {n} words  stream {total} words   from rows {spread(t_new)} ms   "
        f"matrix ({matrix_bytes / 2**20:.0f} MiB) + compress {spread(t_base)} ms   {verdict(t_new, t_base)}")


say(f"{lib.wah_version().decode()}  min .. max over {1 if trace else REPS} repetitions in turn after a warm-up, device events around each way; uniform random keys")
for n_values in ((256,) if trace else VALUES):
    row(n_values)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

"""One call over an operand list (wah_bitop_list_indexed_device) against the only way to answer the same query without it: a
chain of wah_bitop_many_indexed_device calls -- 8 operands, then the running result plus 7 more per call -- on the same
operands, in the same process.  K in {16, 64, 256} columns of 32 MiB OR-ed, for three kinds of column:
  random  -- a 256-bin equality index over uniformly random keys (every bin sparse: literals between short zero fills);
  blocks  -- the same over keys sorted inside blocks of 2^20 rows (every bin clustered: a few words per segment);
  mixed   -- column_spec()'s columns (sparse / clustered / dense in turn);
and AND over 64 mixed columns.  The chain is timed twice: with every intermediate length read back to the host, so that the
library can choose its run-merge route for it (a host round trip per call), and with capacities instead of lengths (no round
trip; every call behind the first then takes the groups route).  Beside each time: the algorithmic bytes -- 4 x (the operands'
words + the result's words), + 8 x n_words for the one decoded intermediate of the list call -- and the fraction of 8 TB/s
they give over the list call's time.
usage: python tools/bitop_list_time.py [random blocks mixed]"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
SEGS = 8457
N = 992 * SEGS  # 8 389 344 words: 32 MiB and a bit
BINS = 256
DEV = "cuda:0"


def timed(run, reps=5):
    run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        run()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def equality_matrix(keys):
    """[BINS, N] int32: row v is the bitmap of keys == v, bit k of the LSB-first stream = row k."""
    m = torch.empty((BINS, N), dtype=torch.int32, device=DEV)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=DEV)
    for v in range(BINS):
        bits = (keys == v).view(N, 4, 8).to(torch.uint8)
        m[v] = (bits * weights).sum(-1).to(torch.uint8).view(torch.int32).view(N)
    return m


def make_matrix(kind):
    if kind == "mixed":
        return wah.columns.make_column_matrix(wah, [wah.columns.column_spec(c, N) for c in range(BINS)], DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(1337)
    keys = torch.randint(0, BINS, (N * 32,), dtype=torch.int16, device=DEV, generator=g)
    if kind == "blocks":
        keys = torch.cat([part.sort().values for part in keys.split(1 << 20)])
    return equality_matrix(keys)


def columns_of(matrix):
    """Every column as a stream and an index of its own (what the chain of the 8-operand call needs to see its operands' lengths)."""
    comp = wah.DeviceCompressor(matrix.numel(), indexed=True)
    stream, _ = wah.columns.compress_column_matrix(comp, matrix)
    starts = comp.seg_offsets[::SEGS].cpu().tolist()
    return [(stream[starts[c]: starts[c + 1]].clone(), (comp.seg_offsets[c * SEGS: (c + 1) * SEGS + 1] - starts[c]).clone()) for c in range(BINS)]


cap = wah.max_compressed_words(N)
n_seg = (cap + 1023) // 1024
scratch = torch.empty(int(lib.wah_bitop_list_scratch_bytes(N, BINS)), dtype=torch.uint8, device=DEV)
outs = [torch.empty(cap, dtype=torch.int32, device=DEV) for _ in range(2)]
offs = [torch.zeros(n_seg + 1, dtype=torch.int64, device=DEV) for _ in range(2)]
sp = torch.cuda.current_stream().cuda_stream


def chain(op, ops, read_back):
    """A op B op ... by calls of at most 8 operands; returns (out, count tensor, out_offsets, calls)."""
    o, c, oo = wah.bitop_many_indexed_device(op, ops[:8], N, scratch=scratch, out=outs[0], out_offsets=offs[0], check=False)
    at, calls = 8, 1
    # (ANDNOT would chain as well: (A and not B ...) and not C ...; AND, OR, XOR are associative)
    while at < len(ops):
        running = o[: int(c.item())] if read_back else o
        o, c, oo = wah.bitop_many_indexed_device(op, [(running, oo)] + ops[at: at + 7], N, scratch=scratch, out=outs[calls & 1],
                                                 out_offsets=offs[calls & 1], check=False)
        at += 7
        calls += 1
    return o, c, oo, calls


def row(kind, op, ops):
    k = len(ops)
    table = wah.bitop_operand_table(ops)
    res = torch.empty(cap, dtype=torch.int32, device=DEV)
    res_offs = torch.zeros(n_seg + 1, dtype=torch.int64, device=DEV)

    def one():
        return wah.bitop_list_indexed_device(op, table, N, scratch=scratch, out=res, out_offsets=res_offs, check=False)

    t_list = [timed(one)]
    assert lib.wah_bitop_list_status(scratch.data_ptr(), N, k, sp) == 0
    t_back = timed(lambda: chain(op, ops, True))
    t_caps = timed(lambda: chain(op, ops, False))
    assert lib.wah_bitop_indexed_status(scratch.data_ptr(), N, sp) == 0
    t_list.append(timed(one))
    _, count, _ = one()
    o, c, oo, calls = chain(op, ops, True)
    torch.cuda.synchronize()
    words = int(count.item())
    same = words == int(c.item()) and torch.equal(res[:words], o[:words]) and torch.equal(res_offs, oo)
    op_words = sum(int(s.numel()) for s, _ in ops)
    nbytes = 4 * (op_words + words) + 8 * N
    best = min(t_list)
    print(f"{kind:6s} {op:3s} K={k:3d}: list {t_list[0]:7.3f} / {t_list[1]:7.3f} ms   chain of {calls:2d} calls: {t_back:7.3f} ms lengths read back, "
          f"{t_caps:7.3f} ms capacities   {op_words / k / n_seg:6.1f} words per operand and segment, result {words} words, "
          f"{nbytes / 1e6:8.1f} MB -> {nbytes / (best * 1e-3) / 8e12:.3f} of 8 TB/s{'' if same else '   RESULTS DIFFER'}", flush=True)


print(f"{lib.wah_version().decode()}  columns of {N} words ({N * 4 / 2**20:.1f} MiB), {BINS} of them per kind", flush=True)
for kind in sys.argv[1:] or ["random", "blocks", "mixed"]:
    matrix = make_matrix(kind)
    ops = columns_of(matrix)
    del matrix
    for k in (16, 64, 256):
        row(kind, "or", ops[:k])
    if kind == "mixed":
        row(kind, "and", ops[:64])
    del ops
    torch.cuda.empty_cache()

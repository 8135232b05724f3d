"""`value IN (set)` over a bit-sliced attribute: the one call (api.bsi_member_device -> wah_bsi_member_indexed_device) against the only
road there was before it --
  old road   columns.values_of_column (8 bytes a row into global memory), torch.isin against the list or a gather from the bit
             array, AND with the existence bits, a pack of the matches into words, DeviceCompressor(indexed=True) over them.
One attribute of 2114 segments (67 106 816 rows, 64 Mi less a ragged end) with an existence bitmap of density 0.9, uniform values of
20 and of 40 bits; the set a sorted list of 2^10 and of 2^20 entries drawn from the values' range, and a bit array of 2^20 bits of
density 0.5 (at 40 bits nearly every value lies beyond it).  Both roads in one process on the same inputs, in turn, REPS times
after one warm-up each, device events around one call; median (min .. max).  Their results must be EQUAL, words and index.  The new
call is timed bare: table, set, output and scratch made before, check=False, the status read after the last repetition.  Beside
the times: the bytes the new call has to move (the slices' stream words in, the decoded bitmap out and in again, the result out)
over its time, and the copy ceiling measured as bench.py --full measures it (wah_copy_device, read + write).
usage: python tools/member_time.py [--label TEXT] [output file]    (default: profiles/member_time.txt)"""
import argparse, importlib, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
c = wah.columns
DEV = "cuda:0"
SEGMENTS = 2114
N = SEGMENTS * 992
ROWS = 32 * N
REPS = 5

ap = argparse.ArgumentParser()
ap.add_argument("--label", default="", help="what was measured (the commit), written into the first line")
ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "member_time.txt"))
args = ap.parse_args()
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


def copy_ceiling():
    src = torch.zeros(ROWS // 4, dtype=torch.int32, device=DEV)
    dst = torch.empty_like(src)
    for _ in range(2):
        wah.copy_device(src, dst)
    ms = timed(lambda: [wah.copy_device(src, dst) for _ in range(5)])[0]
    return 5 * 8.0 * src.numel() / (ms * 1e-3) / 1e9


WEIGHTS = torch.ones(32, dtype=torch.int64, device=DEV) << torch.arange(32, dtype=torch.int64, device=DEV)
compressor = wah.DeviceCompressor(N, device=DEV, indexed=True)


def old_road(bsi, members, words, set_bits):
    values, have = c.values_of_column(wah, bsi)
    if words is None:
        match = torch.isin(values, members)
    else:
        inside = (values >= 0) & (values < set_bits)
        at = torch.where(inside, values, torch.zeros_like(values))
        match = inside & (((words[at >> 5].to(torch.int64) >> (at & 31)) & 1) != 0)
    match &= have
    packed = (match.view(N, 32).to(torch.int64) * WEIGHTS).sum(1)
    compressor.run(torch.where(packed >= 1 << 31, packed - (1 << 32), packed).to(torch.int32))
    return compressor.result(), compressor.seg_offsets


def case(name, bsi, table, members=None, words=None, set_bits=None):
    n_bits = bsi[3]
    scratch = torch.empty(int(lib.wah_bsi_member_scratch_bytes(N, n_bits)), dtype=torch.uint8, device=DEV)
    out = torch.empty(wah.max_compressed_words(N), dtype=torch.int32, device=DEV)
    offs = torch.zeros(SEGMENTS + 1, dtype=torch.int64, device=DEV)
    kw = dict(members=members) if words is None else dict(members=words, bitset=True, set_bits=set_bits)

    def new_call():
        return wah.bsi_member_device(table, n_words=N, exists=True, scratch=scratch, out=out, out_offsets=offs, check=False, **kw)

    _, count, _ = new_call()  # warm-up, and the roads agree
    old, old_offs = old_road(bsi, members, words, set_bits)
    torch.cuda.synchronize()
    assert lib.wah_bsi_member_status(scratch.data_ptr(), N, n_bits, None) == 0
    words_out = int(count.item())
    assert words_out == old.numel() and torch.equal(out[:words_out], old) and torch.equal(offs, old_offs[: SEGMENTS + 1]), f"{name}: the roads DIFFER"
    ts = {"one call": [], "old road": []}
    for _ in range(REPS):
        ts["one call"].append(timed(new_call)[0])
        ts["old road"].append(timed(lambda: old_road(bsi, members, words, set_bits))[0])
    assert lib.wah_bsi_member_status(scratch.data_ptr(), N, n_bits, None) == 0
    one, road = statistics.median(ts["one call"]), statistics.median(ts["old road"])
    moved = 4 * bsi[0].numel() + 8 * N + 4 * words_out
    say(f"{name}: result {words_out} words")
    say(f"    one call   {show(ts['one call'])}")
    say(f"    old road   {show(ts['old road'])}")
    say(f"    the call moves at least {moved / 1e6:.1f} MB (slices in, decoded bitmap out and in, result out): {moved / (one * 1e-3) / 1e9:.0f} GB/s "
        f"({moved / (one * 1e-3) / 1e9 / ceiling:.2f} of the copy ceiling)")
    if one <= road:
        say(f"    old road / one call: {road / one:.1f}")
    else:
        say(f"    one call SLOWER than the old road by {one - road:.3f} ms (spread of its repetitions {max(ts['one call']) - min(ts['one call']):.3f} ms)")


say(f"{lib.wah_version().decode()}  {args.label}  value IN (set) over an attribute of {SEGMENTS} segments ({ROWS} rows) with an existence bitmap: median "
    f"(min .. max) over {REPS} repetitions, the roads in turn, device events around one call after one warm-up")
ceiling = copy_ceiling()
say(f"copy ceiling (wah_copy_device over {ROWS} bytes, read + write, as bench.py --full measures it): {ceiling:.0f} GB/s")
for n_bits in (20, 40):
    gen = torch.Generator(device=DEV).manual_seed(1337 + n_bits)
    wide = (torch.randint(0, 1 << 32, (ROWS,), dtype=torch.int64, device=DEV, generator=gen) << 31) | torch.randint(0, 1 << 31, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    v = wide >> (63 - n_bits)
    del wide
    exists = torch.rand(ROWS, device=DEV, generator=gen) < 0.9
    bsi = c.bsi_from_values(wah, v, n_bits, n_words_per_column=N, exists=exists)
    table = c.column_operand_table(bsi[0], bsi[1], N, list(range(n_bits + 1)))
    for log2 in (10, 20):
        members = torch.sort(v[torch.randint(0, ROWS, (1 << log2,), device=DEV, generator=gen)])[0].contiguous()
        case(f"{n_bits} bits, uniform values, a list of 2^{log2} entries (present values)", bsi, table, members=members)
        del members
    set_bits = 1 << 20
    words = torch.randint(-(1 << 31), 1 << 31, (set_bits // 32,), dtype=torch.int64, device=DEV, generator=gen).to(torch.int32)
    case(f"{n_bits} bits, uniform values, a bit array of 2^20 bits, density 0.5", bsi, table, words=words, set_bits=set_bits)
    del v, exists, bsi, table, words
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")

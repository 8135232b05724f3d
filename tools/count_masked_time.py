"""The histogram of the rows a filter selects (wah_count_masked_indexed_device: one call, no bitmap written) against the only way
to the same numbers without it: wah_bitop_indexed_device("and", column j, filter) once per column into preallocated outputs with
their indexes, then one wah_count_list_indexed_device over the 64 results -- on the same operands, in the same process, every
table and output made before the clock starts.  Bitmaps of 32 MiB and 1 GiB.  Operands: 64 columns with seeds of their own,
uniform with p = 2^-10, uniform with p = 0.01, or clustered (runs of mean 4096 bits).  Masks: uniform 2^-10, uniform 0.5,
clustered, and a mask whose second half is empty (uniform 0.5 in front of zeros).  Every way is timed REPS times in turn (each
time the mean over INNER calls between two events, after a warm-up); min and max are printed -- the spread a difference has to
exceed -- and both ways must give the same 64 numbers.  Beside the times: the words of the 64 operands and of the mask, and the
rate of the new call over 4 x (the operands' words + the mask's words), the streams it is given (it reads the mask once per chunk
of operands that share an image: 4 times for the 32 MiB bitmaps, once for the 1 GiB ones).
usage: python tools/count_masked_time.py [output file] [small large]      (default: profiles/r08_count_masked.txt, both sizes)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
SIZES = {"small": 992 * 8457, "large": 992 * 270600}  # 32 MiB and 1 GiB, whole segments
OPERANDS = [("uniform 2^-10", 2.0 ** -10), ("uniform 0.01", 0.01), ("clustered", None)]
MASKS = [("uniform 2^-10", 2.0 ** -10), ("uniform 0.5", 0.5), ("clustered", None), ("one empty half", "half")]
COLUMNS = 64
REPS = 5

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0] not in SIZES else os.path.join(ROOT, "profiles", "r08_count_masked.txt")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(run, inner):
    run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(inner):
        run()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / inner


def in_turn(ways, inner):
    times = {name: [] for name in ways}
    for _ in range(REPS):
        for name, run in ways.items():
            times[name].append(timed(run, inner))
    return times


def spread(ts):
    return f"{min(ts):9.3f} .. {max(ts):9.3f}"


def verdict(new, base):
    if max(new) < min(base):
        return f"new call faster, {min(base) / max(new):.1f}x at the least"
    if min(new) > max(base):
        return f"new call SLOWER, {min(new) / max(base):.1f}x at the least"
    return "within the spread"


def generate(p, n, seed, out):
    if p is None:
        return wah.gen_clustered_device(n, seed, 4096, device=DEV, out=out)
    if p == "half":
        wah.gen_uniform_device(n, seed, 0.5, device=DEV, out=out)
        out[n // 2:] = 0
        return out
    return wah.gen_uniform_device(n, seed, p, device=DEV, out=out)


def rows(size, n):
    comp = wah.DeviceCompressor(n, indexed=True)
    bitmap = torch.empty(n, dtype=torch.int32, device=DEV)
    n_seg = (wah.max_compressed_words(n) + 1023) // 1024
    sp = torch.cuda.current_stream().cuda_stream
    select_scratch = torch.empty(int(lib.wah_select_scratch_bytes(n, COLUMNS)), dtype=torch.uint8, device=DEV)
    bitop_scratch = torch.empty(int(lib.wah_bitop_indexed_scratch_bytes(n)), dtype=torch.uint8, device=DEV)

    def column(p, seed):
        generate(p, n, seed, bitmap)
        comp.run(bitmap)
        return comp.result().clone(), comp.seg_offsets.clone()

    masks = [(kind, column(p, 4242 + k)) for k, (kind, p) in enumerate(MASKS)]
    for op_kind, p in OPERANDS:
        cols = [column(p, 1337 + j) for j in range(COLUMNS)]
        table = wah.bitop_operand_table(cols)
        op_words = sum(int(s.numel()) for s, _ in cols)
        for mask_kind, mask in masks:
            mask_table = wah.bitop_operand_table([mask])
            mask_words = int(mask[0].numel())
            # the parent route's outputs: an AND has at most the words of both operands in every segment
            caps = [min(wah.max_compressed_words(n), int(s.numel()) + mask_words) + 1 for s, _ in cols]
            outs = [torch.empty(c, dtype=torch.int32, device=DEV) for c in caps]
            out_offs = [torch.zeros(n_seg + 1, dtype=torch.int64, device=DEV) for _ in cols]
            out_words = torch.zeros(COLUMNS, dtype=torch.int64, device=DEV)
            result_table = wah.bitop_operand_table(list(zip(outs, out_offs)))
            new_counts = torch.empty((1, COLUMNS), dtype=torch.int64, device=DEV)
            base_counts = torch.empty(COLUMNS, dtype=torch.int64, device=DEV)

            def new():
                wah.count_masked_device(mask_table, table, n, scratch=select_scratch, counts=new_counts, check=False)

            def base():
                for j, (s, o) in enumerate(cols):
                    rc = lib.wah_bitop_indexed_device(0, n, s.data_ptr(), s.numel(), o.data_ptr(), mask[0].data_ptr(), mask_words, mask[1].data_ptr(),
                                                      outs[j].data_ptr(), caps[j], out_words.data_ptr() + 8 * j, out_offs[j].data_ptr(),
                                                      bitop_scratch.data_ptr(), bitop_scratch.numel(), sp)
                    assert rc == 0, lib.wah_last_error()
                wah.count_device(result_table, n, scratch=select_scratch, counts=base_counts, check=False)

            base()
            assert lib.wah_bitop_indexed_status(bitop_scratch.data_ptr(), n, sp) == 0 and lib.wah_select_status(select_scratch.data_ptr(), sp) == 0
            new()
            assert lib.wah_select_status(select_scratch.data_ptr(), sp) == 0
            assert torch.equal(new_counts.view(-1), base_counts), "COUNTS DIFFER"
            t = in_turn({"new": new, "base": base}, 1 if n > SIZES["small"] else 3)
            assert lib.wah_select_status(select_scratch.data_ptr(), sp) == 0 and torch.equal(new_counts.view(-1), base_counts), "COUNTS DIFFER"
            read = 4 * (op_words + mask_words)
            say(f"{size} {n * 4 / 2**20:.0f} MiB  operands {op_kind:13s} ({op_words} words)  mask {mask_kind:14s} ({mask_words} words, "
                f"{int(new_counts.sum().item())} rows counted)   new {spread(t['new'])} ms   64 x AND + count {spread(t['base'])} ms   "
                f"{verdict(t['new'], t['base'])}   ({read / (min(t['new']) * 1e-3) / 1e9:.1f} GB/s over the streams' words)")
            del outs, out_offs, result_table
        del cols, table
        torch.cuda.empty_cache()


say(f"{lib.wah_version().decode()}  min .. max over {REPS} repetitions in turn, each the mean over 1 or 3 calls between two events; {COLUMNS} operands, 1 mask")
for size in args or list(SIZES):
    rows(size, SIZES[size])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

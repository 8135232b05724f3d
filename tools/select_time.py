"""Counting the set bits of compressed bitmaps and listing their positions (wah_count_list_indexed_device,
wah_positions_indexed_device) against the best a caller has without them: wah_decompress_segments_device into a whole bitmap,
then torch over it -- for a count the word-parallel popcount (shifts, masks and one sum), for positions torch.nonzero over the
unpacked bits, in pieces of 2^30 bits written into an output of the known size.  Bitmaps of 32 MiB and 1 GiB: uniform with
p = 2^-13, 2^-10, 0.01, 0.5 and clustered (runs of mean 4096 bits).  Per bitmap:
  count of 1       one operand;
  count of 256     256 columns of the same kind with seeds of their own in one call, against 256 decodes and popcounts (where 256
                   streams would not fit into 32 GiB: the one column named 256 times, and the row says so);
  positions, all   every set bit (8 bytes out per bit);
  positions, 1000  the 1000 bits from rank total / 2 on -- the baseline has no ranks, it decodes and lists everything and slices.
Every way is timed REPS times in turn (each time the mean over INNER calls between two events, after a warm-up); min and max are
printed -- the spread a difference has to exceed -- and both ways must give the same numbers.  Beside the count of 1: its rate
over the stream's 4 C bytes, and the rate of the decoder's sums pass (wah_decompress_scan_device) over the same stream.
usage: python tools/select_time.py [output file] [small large]      (default: profiles/r07_select.txt, both sizes)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
SIZES = {"small": 992 * 8457, "large": 992 * 270600}  # 32 MiB and 1 GiB, whole segments
KINDS = [("uniform 2^-13", 2.0 ** -13), ("uniform 2^-10", 2.0 ** -10), ("uniform 0.01", 0.01), ("uniform 0.5", 0.5), ("clustered", None)]
COLUMNS = 256
REPS = 5
PIECE = 1 << 25  # words per piece of the baseline's position list: 2^30 bits

args = sys.argv[1:]
out_path = args.pop(0) if args and args[0] not in SIZES else os.path.join(ROOT, "profiles", "r07_select.txt")
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


def generate(kind, p, n, seed, out):
    if p is None:
        return wah.gen_clustered_device(n, seed, 4096, device=DEV, out=out)
    return wah.gen_uniform_device(n, seed, p, device=DEV, out=out)


def popcount_words(x):
    """Set bits of an int32 tensor: the word-parallel popcount, byte sums at the end."""
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return x.view(torch.uint8).sum(dtype=torch.int64)


SHIFTS = torch.arange(8, dtype=torch.uint8, device=DEV)


def list_positions(words, out):
    """Positions of the set bits of an int32 tensor into out (its size is the bitmap's count); returns the number written."""
    at = 0
    for w0 in range(0, words.numel(), PIECE):
        piece = words[w0: w0 + PIECE].view(torch.uint8)
        idx = ((piece[:, None] >> SHIFTS) & 1).view(-1).nonzero().view(-1)
        out[at: at + idx.numel()] = idx + 32 * w0
        at += idx.numel()
    return at


def bitmap_rows(size, n):
    comp = wah.DeviceCompressor(n, indexed=True)
    bitmap = torch.empty(n, dtype=torch.int32, device=DEV)
    decoded = torch.empty(n + 1, dtype=torch.int32, device=DEV)
    seg_ws = torch.empty(int(lib.wah_decompress_segments_workspace_bytes()), dtype=torch.uint8, device=DEV)
    scratch = torch.empty(int(lib.wah_select_scratch_bytes(n, COLUMNS)), dtype=torch.uint8, device=DEV)
    sp = torch.cuda.current_stream().cuda_stream
    for kind, p in KINDS:
        def column(seed):
            generate(kind, p, n, seed, bitmap)
            comp.run(bitmap)
            return comp.result().clone(), comp.seg_offsets.clone()

        stream, offs = column(1337)
        c_words = int(stream.numel())
        own = COLUMNS * 4 * c_words <= 32 << 30
        many = [(stream, offs)] + [column(1338 + j) for j in range(COLUMNS - 1)] if own else [(stream, offs)] * COLUMNS
        table1, table256 = wah.bitop_operand_table([(stream, offs)]), wah.bitop_operand_table(many)
        counts1 = torch.empty(1, dtype=torch.int64, device=DEV)
        counts256 = torch.empty(COLUMNS, dtype=torch.int64, device=DEV)
        base256 = torch.empty(COLUMNS, dtype=torch.int64, device=DEV)

        def decode(op):
            return wah.decompress_segments_device(op[0], op[1], n, out=decoded, workspace=seg_ws, check=False)

        def base_count256():
            for j, op in enumerate(many):
                base256[j] = popcount_words(decode(op))

        total = int(wah.count_device(table1, n, scratch=scratch).item())
        assert total == int(popcount_words(decode((stream, offs))).item()), "COUNTS DIFFER"
        heavy = n > SIZES["small"]
        say(f"{size} {kind}: {n} words ({n * 4 / 2**20:.0f} MiB), stream {c_words} words ({c_words * 4 / 2**20:.2f} MiB), {total} set bits")

        # count of 1, and the rates over the stream's bytes
        t = in_turn({"new": lambda: wah.count_device(table1, n, scratch=scratch, counts=counts1, check=False),
                     "base": lambda: popcount_words(decode((stream, offs)))}, 3 if heavy else 10)
        scan_ws = torch.zeros(int(lib.wah_decompress_workspace_bytes(c_words, 0)), dtype=torch.uint8, device=DEV)
        info = torch.zeros(2, dtype=torch.int64, device=DEV)
        t_scan = in_turn({"scan": lambda: lib.wah_decompress_scan_device(stream.data_ptr(), c_words, info.data_ptr(), scan_ws.data_ptr(), scan_ws.numel(), sp)},
                         3 if heavy else 10)["scan"]
        assert lib.wah_select_status(scratch.data_ptr(), sp) == 0 and lib.wah_decompress_status(scan_ws.data_ptr(), sp) == 0
        say(f"  count of 1       new {spread(t['new'])} ms   decode + popcount {spread(t['base'])} ms   {verdict(t['new'], t['base'])}")
        say(f"                   count call {4 * c_words / (min(t['new']) * 1e-3) / 1e9:8.1f} GB/s over 4 C bytes, "
            f"sums pass {4 * c_words / (min(t_scan) * 1e-3) / 1e9:8.1f} GB/s ({spread(t_scan)} ms)")
        del scan_ws

        # count of 256
        t = in_turn({"new": lambda: wah.count_device(table256, n, scratch=scratch, counts=counts256, check=False), "base": base_count256}, 1 if heavy else 2)
        assert lib.wah_select_status(scratch.data_ptr(), sp) == 0 and torch.equal(counts256, base256), "COUNTS DIFFER"
        words256 = sum(int(s.numel()) for s, _ in many)
        say(f"  count of 256     new {spread(t['new'])} ms   256 x (decode + popcount) {spread(t['base'])} ms   {verdict(t['new'], t['base'])}   "
            f"({'256 columns' if own else 'ONE column named 256 times'}, {4 * words256 / (min(t['new']) * 1e-3) / 1e9:.1f} GB/s over their words)")
        del many, table256

        # positions: all, and a window of 1000
        try:
            out_new = torch.empty(max(total, 1), dtype=torch.int64, device=DEV)
            out_base = torch.empty(max(total, 1), dtype=torch.int64, device=DEV)
            first = total // 2

            def new_all():
                return wah.positions_device(stream, offs, n, out=out_new, scratch=scratch, check=False)

            def new_window():
                return wah.positions_device(stream, offs, n, first=first, out=out_new[:1000], scratch=scratch, check=False)

            def base_all():
                return list_positions(decode((stream, offs)), out_base)

            inner = 1 if heavy else 3
            t = in_turn({"new": new_all, "base": base_all}, inner)
            _, pinfo = new_all()
            assert base_all() == total
            torch.cuda.synchronize()
            assert pinfo.cpu().tolist() == [total, total] and torch.equal(out_new[:total], out_base[:total]), "POSITIONS DIFFER"
            say(f"  positions, all   new {spread(t['new'])} ms   decode + nonzero {spread(t['base'])} ms   {verdict(t['new'], t['base'])}   "
                f"({8 * total / (min(t['new']) * 1e-3) / 1e9:.1f} GB/s of positions)")
            tw = in_turn({"new": new_window}, 3 if heavy else 10)["new"]
            _, pinfo = new_window()
            torch.cuda.synchronize()
            want = min(1000, total - first)
            assert pinfo.cpu().tolist() == [total, want] and torch.equal(out_new[:want], out_base[first: first + want]), "WINDOWS DIFFER"
            say(f"  positions, 1000  new {spread(tw)} ms   decode + nonzero + slice: the row above, {spread(t['base'])} ms   {verdict(tw, t['base'])}")
            del out_new, out_base
        except torch.cuda.OutOfMemoryError as e:
            say(f"  positions        not measured: out of memory ({str(e).splitlines()[0]})")
        assert lib.wah_select_status(scratch.data_ptr(), sp) == 0
        torch.cuda.empty_cache()


say(f"{lib.wah_version().decode()}  min .. max over {REPS} repetitions in turn, each the mean over 1 to 10 calls between two events")
for size in args or list(SIZES):
    bitmap_rows(size, SIZES[size])
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

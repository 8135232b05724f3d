"""Deleting or keeping the rows a bitmap selects from a whole index: the one call (wah_compact_indexed_device through
api.compact_device) against the only road there is without it, a script of existing calls --
  api.decompress_segments_device of the mask and of every column, the words unpacked into one bool per row with torch, boolean
  selection, the survivors packed into words again, and the packed matrix through DeviceCompressor (compress_device).
An index of 64 columns of 1024 segments (32 505 856 rows), its columns uniform at two densities; masks that keep 99.9 %, 50 % and
0.1 % of the rows.  Both roads are timed in turn, REPS times, between two device events after a warm-up, into buffers made
beforehand; the table gives the median and min .. max.  Both roads must give the same stream and the same index.  Every GPU step
runs under a time limit of its own (a watchdog thread ends the process when a step overruns it).

usage: python tools/compact_time.py [--out FILE.txt] [--columns 64] [--segments 1024] [--label TEXT]"""
import argparse
import faulthandler
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5
SEG_WORDS = 992


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_time.txt"))
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--segments", type=int, default=1024)
    ap.add_argument("--label", default="", help="what was measured (the commit), written into the first line")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a single GPU step may take")
    args = ap.parse_args()

    import torch

    wah = importlib.import_module("gpu-wah_amd")
    lib = wah.lib()
    cols = wah.columns
    dev = "cuda:0"
    k, n = args.columns, args.segments * SEG_WORDS
    n_rows = 32 * n

    def step(run, limit=None):
        """One GPU step under its own time limit: the watchdog ends the process if it overruns."""
        faulthandler.dump_traceback_later(limit or args.step_limit, exit=True)
        try:
            got = run()
            torch.cuda.synchronize()
        finally:
            faulthandler.cancel_dump_traceback_later()
        return got

    def timed(run):
        run()  # warm-up
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        got = run()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), got

    def index_of(matrix):
        comp = wah.DeviceCompressor(matrix.numel(), device=dev, indexed=True)
        stream, _ = cols.compress_column_matrix(comp, matrix)
        return stream.clone(), comp.seg_offsets.clone()

    shifts = torch.arange(32, dtype=torch.int32, device=dev)
    weights = torch.ones(32, dtype=torch.int64, device=dev) << torch.arange(32, dtype=torch.int64, device=dev)

    def unpack(words):  # one bool per row
        return ((words.unsqueeze(1) >> shifts) & 1).bool().view(-1)

    lines = [f"{lib.wah_version().decode()}  {args.label}  keep the rows a mask selects of {k} columns of {args.segments} segments ({n_rows} rows): "
             f"median (min .. max) over {REPS} repetitions, the two roads in turn, device events around one call after one warm-up"]
    print(lines[0], flush=True)

    for density in (0.5, 0.001):
        matrix = torch.empty((k, n), dtype=torch.int32, device=dev)
        for c in range(k):
            wah.gen_uniform_device(n, 1000 + c, density, device=dev, out=matrix[c])
        stream, offsets = step(lambda: index_of(matrix), 300)
        del matrix
        table = cols.column_operand_table(stream, offsets, n, list(range(k)))
        for kept in (0.999, 0.5, 0.001):
            mask_words = wah.gen_uniform_device(n, 77, kept, device=dev).view(1, n)
            mask = step(lambda: index_of(mask_words))
            del mask_words
            scratch = torch.empty(int(lib.wah_compact_scratch_bytes(n, n, k)), dtype=torch.uint8, device=dev)
            out = torch.empty(k * wah.max_compressed_words(n), dtype=torch.int32, device=dev)
            out_offsets = torch.empty(k * args.segments + 1, dtype=torch.int64, device=dev)
            out_rows = torch.empty(1, dtype=torch.int64, device=dev)
            packed = torch.empty((k, n), dtype=torch.int32, device=dev)
            comp = wah.DeviceCompressor(packed.numel(), device=dev, indexed=True)

            def one_call():
                return wah.compact_device(mask, table, n, n_rows, n, scratch=scratch, out=out, out_offsets=out_offsets, out_rows=out_rows, check=False)

            def script():
                chosen = unpack(wah.decompress_segments_device(mask[0], mask[1], n))
                for c in range(k):
                    bits = unpack(wah.decompress_segments_device(stream, offsets[c * args.segments:], n))[chosen]
                    padded = torch.zeros(n_rows, dtype=torch.int64, device=dev)
                    padded[: bits.numel()] = bits
                    words = (padded.view(n, 32) * weights).sum(1)
                    packed[c].copy_(torch.where(words >= 1 << 31, words - (1 << 32), words))
                comp.run(packed.view(-1))
                return comp

            times = {"one": [], "script": []}
            for _ in range(REPS):
                t, got = step(lambda: timed(one_call))
                times["one"].append(t)
                t, want = step(lambda: timed(script), 600)
                times["script"].append(t)
            assert lib.wah_compact_status(scratch.data_ptr(), None) == 0
            words_out = int(got[1].item())
            want_stream = want.result()
            same = words_out == want_stream.numel() and torch.equal(got[0][:words_out], want_stream) and torch.equal(got[2], want.seg_offsets[: out_offsets.numel()])
            assert same, ("RESULTS DIFFER", density, kept)
            med = {name: statistics.median(v) for name, v in times.items()}
            line = (f"columns at density {density:<6} mask keeps {100 * kept:5.1f} % ({int(out_rows.item())} rows): one call {med['one']:9.3f} ms "
                    f"({min(times['one']):.3f} .. {max(times['one']):.3f})   decode route {med['script']:9.3f} ms ({min(times['script']):.3f} .. "
                    f"{max(times['script']):.3f})   decode route / one call {med['script'] / med['one']:.2f}   {stream.numel()} words in, {words_out} words out")
            print(line, flush=True)
            lines.append(line)
            del scratch, out, out_offsets, packed, comp, mask
            torch.cuda.empty_cache()
        del stream, offsets, table
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Updating the rows a bitmap selects across a whole index: the one call (wah_update_indexed_device through api.update_device)
against the composition of existing calls that gives the same index --
  per column, with a column on the then side: `else ANDNOT mask`, `then AND mask` and the OR of the two, three
  wah_bitop_list_indexed_device calls; with a constant on the then side one call, `else OR mask` for 1 and `else ANDNOT mask` for
  0; each call writes a decoded bitmap and runs the compress passes over it.  Then the host stitches the columns' streams and
  their shifted indexes into one column matrix, for which it reads every column's word count.
(n_rows is 32 * n_words here and the masks hold nothing behind it, so the composition is spared the further mask it would
otherwise need to keep the rows at or behind n_rows out.)
An index of 64 columns of 1024 segments (32 505 856 rows), its columns uniform at two densities; masks that select 99.9 %, 50 %
and 0.1 % of the rows; the then side once a second index of the same density and once constants, 0 and 1 in turn.  Both roads are
timed in turn, REPS times, between two device events after a warm-up, into buffers and tables made beforehand; the table gives the
median and min .. max.  Both roads must give the same stream and the same index.  Every GPU step runs under a time limit of its
own (a watchdog thread ends the process when a step overruns it).

usage: python tools/update_time.py [--out FILE.txt] [--columns 64] [--segments 1024] [--label TEXT]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_time.txt"))
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
    k, segs = args.columns, args.segments
    n = segs * SEG_WORDS
    n_rows = 32 * n
    cap = wah.max_compressed_words(n)

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

    def uniform_index(seed, density):
        matrix = torch.empty((k, n), dtype=torch.int32, device=dev)
        for c in range(k):
            wah.gen_uniform_device(n, seed + c, density, device=dev, out=matrix[c])
        return step(lambda: index_of(matrix), 300)

    def words(count):
        return torch.empty(int(count), dtype=torch.int32, device=dev)

    def entries(count):
        return torch.empty(int(count), dtype=torch.int64, device=dev)

    lines = [f"{lib.wah_version().decode()}  {args.label}  update the rows a mask selects of {k} columns of {segs} segments ({n_rows} rows): "
             f"median (min .. max) over {REPS} repetitions, the two roads in turn, device events around one road after one warm-up"]
    print(lines[0], flush=True)

    for density in (0.5, 0.001):
        else_stream, else_offsets = uniform_index(1000, density)
        then_stream, then_offsets = uniform_index(5000, density)
        else_table = cols.column_operand_table(else_stream, else_offsets, n, list(range(k)))
        then_columns = cols.column_operand_table(then_stream, then_offsets, n, list(range(k)))
        bits = [c & 1 for c in range(k)]
        then_constants = wah.update_operand_table(bits, device=dev)
        for selected in (0.999, 0.5, 0.001):
            mask_words = wah.gen_uniform_device(n, 77, selected, device=dev).view(1, n)
            mask = step(lambda: index_of(mask_words))
            del mask_words
            mask_row = wah.bitop_operand_table([mask])
            scratch = torch.empty(int(lib.wah_update_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
            out, out_offsets = words(k * cap), entries(k * segs + 1)
            # the composition's buffers: three results of one bitmap each, the tables of its calls, and the stitched whole
            list_scratch = torch.empty(int(lib.wah_bitop_list_scratch_bytes(n, 2)), dtype=torch.uint8, device=dev)
            tmp = [(words(cap), entries(segs + 1)) for _ in range(3)]
            keep = [torch.cat([else_table[c: c + 1], mask_row]) for c in range(k)]   # else ANDNOT mask / else OR mask
            take = [torch.cat([then_columns[c: c + 1], mask_row]) for c in range(k)]  # then AND mask
            both = wah.bitop_operand_table(tmp[:2])
            whole, whole_offsets = words(k * cap), entries(k * segs + 1)

            for name, then_table in (("a second index", then_columns), ("constants", then_constants)):
                constants = then_table is then_constants

                def one_call():
                    return wah.update_device(mask_row, else_table, then_table, n, n_rows, scratch=scratch, out=out, out_offsets=out_offsets, check=False)

                def composition():
                    at = 0
                    for c in range(k):
                        if constants:
                            last = 0
                            got = wah.bitop_list_indexed_device("or" if bits[c] else "andnot", keep[c], n, scratch=list_scratch, out=tmp[0][0],
                                                                out_offsets=tmp[0][1], check=False)
                        else:
                            last = 2
                            wah.bitop_list_indexed_device("andnot", keep[c], n, scratch=list_scratch, out=tmp[0][0], out_offsets=tmp[0][1], check=False)
                            wah.bitop_list_indexed_device("and", take[c], n, scratch=list_scratch, out=tmp[1][0], out_offsets=tmp[1][1], check=False)
                            got = wah.bitop_list_indexed_device("or", both, n, scratch=list_scratch, out=tmp[2][0], out_offsets=tmp[2][1], check=False)
                        count = int(got[1].item())  # the stitching needs every column's length on the host
                        whole[at: at + count].copy_(tmp[last][0][:count])
                        torch.add(tmp[last][1][:segs], at, out=whole_offsets[c * segs: (c + 1) * segs])
                        at += count
                    whole_offsets[k * segs] = at
                    return at

                times = {"one": [], "composition": []}
                for _ in range(REPS):
                    t, got = step(lambda: timed(one_call))
                    times["one"].append(t)
                    t, total = step(lambda: timed(composition), 600)
                    times["composition"].append(t)
                assert lib.wah_update_status(scratch.data_ptr(), None) == 0
                words_out = int(got[1].item())
                same = words_out == total and torch.equal(got[0][:words_out], whole[:total]) and torch.equal(got[2], whole_offsets)
                assert same, ("RESULTS DIFFER", density, selected, name)
                med = {road: statistics.median(v) for road, v in times.items()}
                line = (f"columns at density {density:<6} mask selects {100 * selected:5.1f} %  then side: {name:<14}: one call {med['one']:9.3f} ms "
                        f"({min(times['one']):.3f} .. {max(times['one']):.3f})   composition {med['composition']:9.3f} ms ({min(times['composition']):.3f} .. "
                        f"{max(times['composition']):.3f})   composition / one call {med['composition'] / med['one']:.2f}   {words_out} words out")
                print(line, flush=True)
                lines.append(line)
            del scratch, out, out_offsets, list_scratch, tmp, keep, take, both, whole, whole_offsets, mask, mask_row
            torch.cuda.empty_cache()
        del else_stream, else_offsets, then_stream, then_offsets, else_table, then_columns, then_constants
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

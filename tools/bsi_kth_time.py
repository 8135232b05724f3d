"""The median and the maximum of a bit-sliced attribute: the one call (wah_bsi_kth_indexed_device, a radix select on the device)
against the only way to get the same answer without it -- a binary search over the value driven from Python, one
columns.range_column (`value <= mid`) and one count (api.count_masked_device under a mask, api.count_device without) per bit of
the value, each with a host round trip for the count.

Attributes of 20 and 32 slices of 32 MiB each (uniform values: every slice is incompressible), with a mask of density 0.01 and
without one.  Both ways are timed in turn, REPS times, between two device events after a warm-up (the one call: the mean over
CALLS calls; the composition: one search, its host round trips included); the table gives the median and min .. max, and both ways
must give the same value.  Beside the times: the bytes of the rows the one call walks, pass by pass (4 x the words of the filters
and of the slices down to the digit's end), and the fraction of 8 TB/s their sum gives over the one call's median.  Every GPU
step runs under a time limit of its own (a watchdog thread ends the process when a step overruns it).

--alternative NAME: the library named by WAH_LIB_PATH is another build of the kernels (`make EXTRA=-DWAH_BSI_KTH_DIGIT_BITS=2`,
`-DWAH_BSI_KTH_COPIES=1`): only the one call is timed, and its rows are merged into the file's "alternatives".
usage: python tools/bsi_kth_time.py [--out FILE.json] [--slices 20 32] [--segments 8457] [--alternative NAME --digit D --copies C]"""
import argparse
import faulthandler
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, CALLS = 5, 3
DIGIT, COPIES = 4, 8  # kBsiKthDigitBits, kBsiKthCopies of the shipped build (gpu-wah_amd/csrc/wah_internal.hpp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsi_kth_time.json"))
    ap.add_argument("--slices", type=int, nargs="*", default=[20, 32])
    ap.add_argument("--segments", type=int, default=8457)  # 8 389 344 words: 32 MiB and a bit per slice
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a single GPU step may take")
    ap.add_argument("--alternative", default=None)
    ap.add_argument("--digit", type=int, default=DIGIT)
    ap.add_argument("--copies", type=int, default=COPIES)
    args = ap.parse_args()

    import torch

    wah = importlib.import_module("gpu-wah_amd")
    lib = wah.lib()
    dev = "cuda:0"
    segs = args.segments
    n = 992 * segs
    cap = wah.max_compressed_words(n)
    n_seg = (cap + 1023) // 1024

    def step(what, run, limit=None):
        """One GPU step under its own time limit: the watchdog ends the process if it overruns."""
        faulthandler.dump_traceback_later(limit or args.step_limit, exit=True)
        try:
            got = run()
            torch.cuda.synchronize()
        finally:
            faulthandler.cancel_dump_traceback_later()
        return got

    def timed(run, calls):
        run()  # warm-up
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(calls):
            run()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / calls

    def build_mask():
        comp = wah.DeviceCompressor(n, device=dev, indexed=True)
        comp.run(wah.gen_uniform_device(n, 77, 0.01, device=dev))
        return comp.result().clone(), comp.seg_offsets.clone()

    mask = step("mask", build_mask)
    range_scratch = torch.empty(int(lib.wah_bitop_indexed_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    select_scratch = torch.empty(int(lib.wah_select_scratch_bytes(n, 1)), dtype=torch.uint8, device=dev)
    rows = []
    print(f"{lib.wah_version().decode()}  slices of {n} words ({n * 4 / 2**20:.1f} MiB), digit {args.digit}, {args.copies} histogram copies; "
          f"median (min .. max) over {REPS} repetitions, the two ways in turn", flush=True)
    for k in args.slices:
        def build():
            matrix = torch.empty((k, n), dtype=torch.int32, device=dev)
            for i in range(k):
                wah.gen_uniform_device(n, 4000 + i, 0.5, device=dev, out=matrix[i])
            comp = wah.DeviceCompressor(matrix.numel(), device=dev, indexed=True)
            stream, _ = wah.columns.compress_column_matrix(comp, matrix)
            return stream, comp.seg_offsets

        stream, seg_offsets = step(f"build {k} slices", build, 300)
        bsi = (stream, seg_offsets, n, k, False)
        starts = seg_offsets[::segs].cpu().tolist()
        slice_words = [starts[i + 1] - starts[i] for i in range(k)]
        slice_table = wah.columns.column_operand_table(stream, seg_offsets, n, list(range(k)))
        mask_row = torch.tensor([[mask[0].data_ptr(), mask[0].numel(), mask[1].data_ptr()]], dtype=torch.int64, device=dev)
        kth_scratch = torch.empty(int(lib.wah_bsi_kth_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
        result = torch.zeros(5, dtype=torch.int64, device=dev)
        range_table = torch.empty((k, 3), dtype=torch.int64, device=dev)
        bounds = torch.empty(2, dtype=torch.int64, device=dev)
        res = torch.empty(cap, dtype=torch.int32, device=dev)
        res_offs = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
        counts = torch.zeros((1, 1), dtype=torch.int64, device=dev)
        for masked in (False, True):
            table = torch.cat([mask_row, slice_table]).contiguous() if masked else slice_table
            n_filters = 1 if masked else 0
            filter_words = int(mask[0].numel()) if masked else 0
            pass_bytes = [4 * (filter_words + sum(slice_words[: min(first + args.digit, k)])) for first in range(0, k, args.digit)]
            for name, num, den in (("median", 1, 2), ("max", 1, 1)):
                query = wah.bsi_kth_query(wah.BSI_KTH_QUANTILE, num, den, dev)

                def one():
                    wah.bsi_kth_device(table, query, n, n_filters, scratch=kth_scratch, result=result, check=False)

                def count_at_most(mid):  # rows of the selection with value <= mid: one sweep, one count, one host read
                    out, _, out_offs = wah.columns.range_column(wah, bsi, 0, mid, table=range_table, bounds=bounds, scratch=range_scratch, out=res,
                                                                out_offsets=res_offs, check=False)
                    if masked:
                        wah.count_masked_device(mask_row, [(out, out_offs)], n, scratch=select_scratch, counts=counts, check=False)
                    else:
                        wah.count_device([(out, out_offs)], n, scratch=select_scratch, counts=counts.view(-1), check=False)
                    return int(counts.item())

                found = {}

                def composed():
                    total = count_at_most((1 << k) - 1)
                    rank = num * (total - 1) // den
                    lo, hi = 0, (1 << k) - 1
                    searches = 1
                    while lo < hi:  # the smallest value with more than `rank` rows at or below it
                        mid = (lo + hi) // 2
                        searches += 1
                        if count_at_most(mid) > rank:
                            hi = mid
                        else:
                            lo = mid + 1
                    found["value"], found["total"], found["steps"] = lo, total, searches

                times = {"one call": [], "composition": []}
                for _ in range(REPS):
                    times["one call"].append(step(f"one call, {k} slices, {name}", lambda: timed(one, CALLS)))
                    assert lib.wah_bsi_kth_status(kth_scratch.data_ptr(), None) == 0
                    if args.alternative is None:
                        times["composition"].append(step(f"composition, {k} slices, {name}", lambda: timed(composed, 1), 300))
                got = [int(v) & ((1 << 64) - 1) for v in result.tolist()]
                row = dict(slices=k, masked=masked, query=name, n_words=n, digit=args.digit, copies=args.copies, value=got[1], total=got[2],
                           pass_bytes=pass_bytes, bytes_walked=sum(pass_bytes), one_call_ms=statistics.median(times["one call"]),
                           one_call_min_ms=min(times["one call"]), one_call_max_ms=max(times["one call"]))
                row["fraction_of_8_TBps"] = row["bytes_walked"] / (row["one_call_ms"] * 1e-3) / 8e12
                line = (f"{k:2d} slices, {'1 % mask' if masked else 'no mask ':8s} {name:6s}: one call {row['one_call_ms']:8.3f} ms "
                        f"({row['one_call_min_ms']:.3f} .. {row['one_call_max_ms']:.3f})   {row['bytes_walked'] / 1e6:.1f} MB walked -> "
                        f"{row['fraction_of_8_TBps']:.3f} of 8 TB/s")
                if args.alternative is None:
                    assert got[0] == 1 and (got[1], got[2]) == (found["value"], found["total"]), ("RESULTS DIFFER", got, found)
                    row.update(composition_ms=statistics.median(times["composition"]), composition_min_ms=min(times["composition"]),
                               composition_max_ms=max(times["composition"]), composition_sweeps=found["steps"])
                    row["ratio"] = row["composition_ms"] / row["one_call_ms"]
                    line += (f"   composition of {found['steps']} sweeps {row['composition_ms']:8.3f} ms ({row['composition_min_ms']:.3f} .. "
                             f"{row['composition_max_ms']:.3f})   ratio {row['ratio']:.1f}")
                rows.append(row)
                print(line + f"   value {got[1]} of {got[2]} rows", flush=True)
        del stream, seg_offsets, bsi, slice_table
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.alternative is None:
        record = dict(version=lib.wah_version().decode(), reps=REPS, calls=CALLS, digit=args.digit, copies=args.copies,
                      timed="device events around CALLS calls (the composition: one search) after one warm-up", rows=rows, alternatives={})
    else:
        with open(args.out) as f:
            record = json.load(f)
        record.setdefault("alternatives", {})[args.alternative] = rows
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

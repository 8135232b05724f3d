"""The values of listed rows of a bit-sliced attribute: the one call (wah_fetch_indexed_device, WAH_FETCH_BITS) against the only
road there is without it -- api.decompress_segments_device of EVERY slice, whole, and a torch gather of the listed rows' bits
out of each decoded slice, a script of existing calls.

Attributes of 20 and 32 slices of 32 MiB each (uniform values: every slice is incompressible); row lists of 100, 10 000, 10^6 and
10^7 rows spread uniformly over the bitmap (sorted, duplicates as they fall), and one list of ALL rows of 64 consecutive
segments.  Both roads are timed in turn, REPS times, between two device events after a warm-up (the mean over CALLS calls each);
the table gives the median and min .. max, and both roads must give the same values.  Beside the times: the items the list is
cut into (at most 64 listed rows of one segment: one walk of the segment each).  Every GPU step runs under a time limit of its
own (a watchdog thread ends the process when a step overruns it).

usage: python tools/fetch_time.py [--out FILE.json] [--slices 20 32] [--segments 8457]"""
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
SEG_BITS = 31744


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fetch_time.json"))
    ap.add_argument("--slices", type=int, nargs="*", default=[20, 32])
    ap.add_argument("--segments", type=int, default=8457)  # 8 389 344 words: 32 MiB and a bit per slice
    ap.add_argument("--lists", type=int, nargs="*", default=[100, 10_000, 1_000_000, 10_000_000])
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a single GPU step may take")
    args = ap.parse_args()

    import torch

    wah = importlib.import_module("gpu-wah_amd")
    lib = wah.lib()
    dev = "cuda:0"
    segs = args.segments
    n = 992 * segs

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

    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    lists = [(f"{count} rows, uniform", torch.sort(torch.randint(0, 32 * n, (count,), generator=gen, device=dev)).values) for count in args.lists]
    first = (segs // 3) * SEG_BITS
    lists.append(("all rows of 64 segments", torch.arange(first, first + 64 * SEG_BITS, device=dev)))
    for _, rows in lists:
        assert int(rows.max()) < 32 * n

    records, lines = [], []
    head = (f"{lib.wah_version().decode()}  slices of {n} words ({n * 4 / 2**20:.1f} MiB); median (min .. max) over {REPS} repetitions of the mean "
            f"of {CALLS} calls, the two roads in turn")
    print(head, flush=True)
    lines.append(head)
    for k in args.slices:
        def build():
            matrix = torch.empty((k, n), dtype=torch.int32, device=dev)
            for i in range(k):
                wah.gen_uniform_device(n, 4000 + i, 0.5, device=dev, out=matrix[i])
            comp = wah.DeviceCompressor(matrix.numel(), device=dev, indexed=True)
            stream, _ = wah.columns.compress_column_matrix(comp, matrix)
            return stream, comp.seg_offsets

        stream, seg_offsets = step(f"build {k} slices", build, 300)
        table = wah.columns.column_operand_table(stream, seg_offsets, n, list(range(k)))
        decoded = torch.empty(wah.decoded_words(wah.max_compressed_words(n)), dtype=torch.int32, device=dev)
        workspace = torch.empty(int(lib.wah_decompress_segments_workspace_bytes()), dtype=torch.uint8, device=dev)
        for name, rows in lists:
            count = int(rows.numel())
            seg_of = rows // SEG_BITS
            heads = torch.ones(count, dtype=torch.bool, device=dev)
            heads[1:] = (seg_of[1:] != seg_of[:-1]) | (torch.arange(1, count, device=dev) % 64 == 0)
            items, touched = int(heads.sum()), int(torch.unique(seg_of).numel())
            scratch = torch.empty(int(lib.wah_fetch_scratch_bytes(n, count)), dtype=torch.uint8, device=dev)
            out = torch.empty(count, dtype=torch.int64, device=dev)
            word, bit = rows >> 5, rows & 31
            values = torch.empty(count, dtype=torch.int64, device=dev)

            def one():
                wah.fetch_device(table, rows, n, wah.FETCH_BITS, scratch=scratch, out=out, check=False)

            def decode_and_gather():
                values.zero_()
                for i in range(k):
                    words = wah.decompress_segments_device(stream, seg_offsets[i * segs: (i + 1) * segs + 1], n, out=decoded, workspace=workspace, check=False)
                    values.bitwise_or_(((words[word].to(torch.int64) >> bit) & 1) << (k - 1 - i))

            times = {"one call": [], "decode": []}
            for _ in range(REPS):
                times["one call"].append(step(f"one call, {k} slices, {name}", lambda: timed(one, CALLS)))
                assert lib.wah_fetch_status(scratch.data_ptr(), None) == 0
                times["decode"].append(step(f"decode and gather, {k} slices, {name}", lambda: timed(decode_and_gather, CALLS), 300))
                assert lib.wah_decompress_status(workspace.data_ptr(), None) == 0
            assert torch.equal(out, values), ("RESULTS DIFFER", k, name)
            row = dict(slices=k, list=name, n_words=n, listed_rows=count, items=items, segments_touched=touched,
                       one_call_ms=statistics.median(times["one call"]), one_call_min_ms=min(times["one call"]), one_call_max_ms=max(times["one call"]),
                       decode_ms=statistics.median(times["decode"]), decode_min_ms=min(times["decode"]), decode_max_ms=max(times["decode"]))
            row["decode_over_one_call"] = row["decode_ms"] / row["one_call_ms"]
            records.append(row)
            line = (f"{k:2d} slices, {name:26s}: one call {row['one_call_ms']:9.3f} ms ({row['one_call_min_ms']:.3f} .. {row['one_call_max_ms']:.3f})   "
                    f"{items} items in {touched} segments   decode + gather {row['decode_ms']:9.3f} ms ({row['decode_min_ms']:.3f} .. "
                    f"{row['decode_max_ms']:.3f})   decode / one call {row['decode_over_one_call']:.2f}")
            print(line, flush=True)
            lines.append(line)
        del stream, seg_offsets, table, decoded
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    record = dict(version=lib.wah_version().decode(), reps=REPS, calls=CALLS, timed="device events around CALLS calls after one warm-up", rows=records)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

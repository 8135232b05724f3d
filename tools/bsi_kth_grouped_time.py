"""MIN / MAX and the median of a bit-sliced attribute PER GROUP: the one call (wah_bsi_kth_grouped_indexed_device, every (group,
query) pair a lane of one radix select) against the same answers by the loop columns.extremes_by runs -- one wah_bsi_kth_indexed_device
call per group and query over the filters, the group's rows and the slices, each with a host read of its result.

2^24 rows (rounded up to whole segments of 992 words); a uniform 20-bit and a uniform 32-bit attribute; keys of 3 x 2 values (two
grouping attributes) and one key of 64 values, in random row order and sorted (clustered: a group's rows are one run); a filter of
density 0.01 and none; the queries {MIN, MAX} and {median}.  Both ways are timed in turn, REPS times, between two device events
after a warm-up (the one call: the mean over CALLS calls; the loop: one run of it, host reads included); the table gives the median
and min .. max, and both ways must give the same results.  Beside the times: the bytes the lanes' items would walk without the
short cut -- per lane and pass 4 x the words of the filters, of the group's rows and of the slices down to the digit's end, the
formula of DESIGN.md 5.14 -- and the fraction of 8 TB/s their sum gives over the one call's median.  Every GPU step runs under a
time limit of its own (a watchdog thread ends the process when a step overruns it).

--alternative NAME: the library named by WAH_LIB_PATH is another build of the kernels (`make EXTRA=-DWAH_BSI_KTH_GROUP_COPIES=8`,
`-DWAH_BSI_KTH_GROUP_SEGMENT_FASTEST`): only the one call is timed, and its lines are appended to the file under that name.
usage: python tools/bsi_kth_grouped_time.py [--out FILE.txt] [--slices 20 32] [--segments 529] [--alternative NAME]"""
import argparse
import faulthandler
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, CALLS = 5, 3
DIGIT = 4  # kBsiKthDigitBits of the shipped build (gpu-wah_amd/csrc/wah_internal.hpp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsi_kth_grouped_time.txt"))
    ap.add_argument("--slices", type=int, nargs="*", default=[20, 32])
    ap.add_argument("--segments", type=int, default=529)  # 524 768 words: 2^24 rows and a bit
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a single GPU step may take")
    ap.add_argument("--alternative", default=None)
    args = ap.parse_args()

    import torch

    wah = importlib.import_module("gpu-wah_amd")
    lib = wah.lib()
    dev = "cuda:0"
    segs = args.segments
    n = 992 * segs
    rows = 32 * n
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

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
    mask_row = torch.tensor([[mask[0].data_ptr(), mask[0].numel(), mask[1].data_ptr()]], dtype=torch.int64, device=dev)
    mask_words = int(mask[1][segs].item())
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    what = "ALTERNATIVE %s: " % args.alternative if args.alternative else ""
    say(f"{what}{lib.wah_version().decode()}  {rows} rows ({n} words, {segs} segments a row); median (min .. max) over {REPS} repetitions, "
        f"the two ways in turn; one call = mean of {CALLS} calls between device events, loop = one run with its host reads")

    key_shapes = (("3 x 2", (3, 2)), ("64", (64,)))
    query_sets = (("min, max", [(wah.BSI_KTH_QUANTILE, 0, 1), (wah.BSI_KTH_QUANTILE, 1, 1)]), ("median", [(wah.BSI_KTH_QUANTILE, 1, 2)]))
    for k in args.slices:
        values = torch.randint(0, 1 << k, (rows,), dtype=torch.int64, device=dev, generator=gen)
        for order in ("random", "sorted"):
            for shape_name, shape in key_shapes:
                def build():
                    keys, indexes = [], []
                    flat = torch.randint(0, int(torch.tensor(shape).prod()), (rows,), dtype=torch.int64, device=dev, generator=gen)
                    if order == "sorted":
                        flat = flat.sort().values
                    for r, count in enumerate(shape):  # row-major: the first key runs slowest
                        div = int(torch.tensor(shape[r + 1:]).prod()) if r + 1 < len(shape) else 1
                        keys.append((flat // div) % count)
                        st, offs, n_key = wah.columns.index_from_keys(wah, keys[-1], count)
                        assert n_key == n
                        indexes.append((st, offs, list(range(count))))
                    # values sorted by key: rows of one group are one run, the values inside it stay uniform
                    bsi = wah.columns.bsi_from_values(wah, values, k)
                    assert bsi[2] == n
                    return indexes, bsi

                indexes, bsi = step(f"build {k} slices, keys {shape_name} {order}", build, 300)
                stream, seg_offsets = bsi[0], bsi[1]
                slice_table = wah.columns.column_operand_table(stream, seg_offsets, n, list(range(k)))
                starts = seg_offsets[:: segs][: k + 1].cpu().tolist()
                slice_words = [starts[i + 1] - starts[i] for i in range(k)]
                _, groups, _ = wah.columns._group_tables(wah, indexes, n, None)
                n_groups, r = int(groups.shape[0]), len(shape)
                group_words = []
                for st, offs, ids in indexes:
                    at = offs[:: segs][: len(ids) + 1].cpu().tolist()
                    group_words.append([at[i + 1] - at[i] for i in range(len(ids))])
                for masked in (False, True):
                    filters = mask_row if masked else None
                    n_front = 1 if masked else 0
                    for q_name, queries in query_sets:
                        n_q = len(queries)
                        d_queries = wah.bsi_kth_queries(queries, dev)
                        scratch = torch.empty(int(lib.wah_bsi_kth_grouped_scratch_bytes(n, k, n_groups, n_q)), dtype=torch.uint8, device=dev)
                        results = torch.zeros((n_groups, n_q, 5), dtype=torch.int64, device=dev)

                        def one():
                            wah.bsi_kth_grouped_device(filters, groups.view(-1, 3), slice_table, d_queries, n, rows_per_group=r, scratch=scratch,
                                                       results=results, check=False)

                        # the loop of extremes_by: one table, the group's rows overwritten in place, one call and one host read per pair
                        table = torch.empty((n_front + r + k, 3), dtype=torch.int64, device=dev)
                        if masked:
                            table[:1] = mask_row
                        table[n_front + r:] = slice_table
                        single = [wah.bsi_kth_query(*q, device=dev) for q in queries]
                        kth_scratch = torch.empty(int(lib.wah_bsi_kth_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
                        looped = []

                        def loop():
                            del looped[:]
                            for g in range(n_groups):
                                table[n_front: n_front + r] = groups[g]
                                for query in single:
                                    looped.append(wah.bsi_kth_device(table, query, n, n_front + r, scratch=kth_scratch).tolist())

                        times = {"one call": [], "loop": []}
                        for _ in range(REPS):
                            times["one call"].append(step("one call", lambda: timed(one, CALLS)))
                            assert lib.wah_bsi_kth_grouped_status(scratch.data_ptr(), None) == 0
                            if args.alternative is None:
                                times["loop"].append(step("loop", lambda: timed(loop, 1), 300))
                        got = results.view(-1, 5).tolist()
                        # bytes: per lane and pass the filters, the group's rows, the slices down to the digit's end
                        passes = [sum(slice_words[: min(first + DIGIT, k)]) for first in range(0, k, DIGIT)]
                        per_group = []
                        for g in range(n_groups):
                            pick, rest = [], g
                            for count in reversed(shape):
                                pick.append(rest % count)
                                rest //= count
                            own = sum(group_words[i][v] for i, v in enumerate(reversed(pick)))
                            per_group.append(sum(4 * ((mask_words if masked else 0) + own + p) for p in passes))
                        walked = n_q * sum(per_group)
                        ms = statistics.median(times["one call"])
                        line = (f"{k:2d} bits, keys {shape_name:5s} {order:6s}, {'1 % filter' if masked else 'no filter ':10s}, {q_name:8s}: {n_groups * n_q:3d} lanes  "
                                f"one call {ms:8.3f} ms ({min(times['one call']):.3f} .. {max(times['one call']):.3f})   "
                                f"{walked / 1e6:9.1f} MB to walk -> {walked / (ms * 1e-3) / 8e12:.3f} of 8 TB/s")
                        if args.alternative is None:
                            assert got == looped, ("RESULTS DIFFER", got[:4], looped[:4])
                            loop_ms = statistics.median(times["loop"])
                            line += (f"   loop of {n_groups * n_q:3d} calls {loop_ms:9.3f} ms ({min(times['loop']):.3f} .. {max(times['loop']):.3f})   "
                                     f"ratio {loop_ms / ms:6.1f}")
                        say(line)
                del indexes, bsi, stream, seg_offsets, slice_table, groups
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.alternative else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

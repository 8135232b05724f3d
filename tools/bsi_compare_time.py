"""`A > B` row by row over two bit-sliced attributes: the one call (columns.compare_columns -> wah_bsi_compare_indexed_device)
against the only way to get the same answer without it -- the sweep composed slice by slice from the existing indexed calls
(chain() below), four calls per significance, each of which writes a decoded bitmap and runs the compress passes over it:
    g  = eq AND a AND NOT b     one clause call of three one-operand clauses (wah_bitop_clauses_indexed_device)
    gt = gt OR g                wah_bitop_indexed_device
    x  = a XOR b                wah_bitop_indexed_device
    eq = eq AND NOT x           wah_bitop_indexed_device
(three for the first significance, where gt is g).  Capacities as lengths, no host round trip, intermediates in a pool of buffers.

Two attributes of 20 and of 40 slices of 32 MiB each (uniform values: every slice is incompressible; the two attributes are
independent, so the rows still equal thin out by half per significance, which the chain's calls profit from and the one call does
not look at).  Both ways are timed in turn, REPS times, each time the mean over CALLS calls between two device events after a
warm-up call (the one call as compare_columns makes it: the row table is rewritten in place each time, which is part of what is
timed); the table gives the median and min .. max -- the spread a difference has to exceed -- and both ways must give the same words
and the same index.  Beside the times: the bytes the one call has to move, 4 x the words of both attributes' rows read + 8 x n_words
for the one decoded bitmap written and read by the compress passes + 4 x the result's words, and the fraction of 8 TB/s they give
over the one call's median.  Every GPU step runs under a time limit of its own (a watchdog thread ends the process when a step
overruns it); everything runs in this one process.
usage: python tools/bsi_compare_time.py [--out FILE.txt] [--slices 20 40] [--segments 8457]"""
import argparse
import faulthandler
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, CALLS = 7, 3


def chain(op2, op_and_andnot, slices_a, slices_b, ones, release=lambda x: None):
    """A > B from the existing calls, most significant slice first.  op2(name, x, y) -> operand with name in "or", "xor", "andnot"
    (andnot: x AND NOT y); op_and_andnot(e, a, b) -> e AND a AND NOT b; release(operand): an intermediate the sweep no longer
    reads.  slices_*: the two attributes' slices, equally many; ones: the all-ones bitmap.  Returns (gt, calls)."""
    eq, gt, calls = ones, None, 0
    for a, b in zip(slices_a, slices_b):
        g = op_and_andnot(eq, a, b)
        calls += 1
        if gt is None:
            gt = g
        else:
            grown = op2("or", gt, g)
            calls += 1
            release(gt)
            release(g)
            gt = grown
        x = op2("xor", a, b)
        kept = op2("andnot", eq, x)
        calls += 2
        release(x)
        if eq is not ones:
            release(eq)
        eq = kept
    return gt, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsi_compare_time.txt"))
    ap.add_argument("--slices", type=int, nargs="*", default=[20, 40])
    ap.add_argument("--segments", type=int, default=8457)  # 8 389 344 words: 32 MiB and a bit per slice
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a single GPU step may take")
    args = ap.parse_args()

    import torch

    wah = importlib.import_module("gpu-wah_amd")
    lib = wah.lib()
    dev = "cuda:0"
    segs = args.segments
    n = 992 * segs
    cap = wah.max_compressed_words(n)
    n_seg = (cap + 1023) // 1024
    sp = None
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def step(what, run, limit=None):
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
        for _ in range(CALLS):
            run()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / CALLS

    scratch = torch.empty(int(lib.wah_bitop_indexed_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    say(f"{lib.wah_version().decode()}  slices of {n} words ({n * 4 / 2**20:.1f} MiB); A > B; median (min .. max) over {REPS} repetitions of "
        f"the mean of {CALLS} calls, the two ways in turn")

    def all_ones():
        comp = wah.DeviceCompressor(n, device=dev, indexed=True)
        comp.run(torch.full((n,), -1, dtype=torch.int32, device=dev))
        return comp.result().clone(), comp.seg_offsets.clone()

    ones = step("all ones", all_ones)
    for k in args.slices:
        def build(seed):
            matrix = torch.empty((k, n), dtype=torch.int32, device=dev)
            for i in range(k):
                wah.gen_uniform_device(n, seed + i, 0.5, device=dev, out=matrix[i])
            comp = wah.DeviceCompressor(matrix.numel(), device=dev, indexed=True)
            stream, _ = wah.columns.compress_column_matrix(comp, matrix)
            return stream.clone(), comp.seg_offsets.clone()

        def own_rows(stream, seg_offsets):  # the chain's operands: every slice as a stream and an index of its own
            starts = seg_offsets[::segs].cpu().tolist()
            return [(stream[starts[i]: starts[i + 1]].clone(), (seg_offsets[i * segs: (i + 1) * segs + 1] - starts[i]).clone()) for i in range(k)]

        attr = [step(f"build {k} slices", lambda seed=seed: build(seed), 300) for seed in (4000, 9000)]
        bsi_a, bsi_b = ((stream, seg_offsets, n, k, False) for stream, seg_offsets in attr)
        slices_a, slices_b = (own_rows(*pair) for pair in attr)
        row_words = int(attr[0][0].numel()) + int(attr[1][0].numel())
        pool = [(torch.empty(cap, dtype=torch.int32, device=dev), torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)) for _ in range(8)]
        slot_of = {id(out): i for i, (out, _) in enumerate(pool)}
        table = torch.empty((2 * k, 3), dtype=torch.int64, device=dev)
        res = torch.empty(cap, dtype=torch.int32, device=dev)
        res_offs = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
        last = {}

        def one():  # (compare_columns as a caller has it: the row table is rewritten in place on every call)
            last["one"] = wah.columns.compare_columns(wah, bsi_a, ">", bsi_b, table=table, scratch=scratch, out=res, out_offsets=res_offs, check=False)

        def chained():
            free = list(range(len(pool)))

            def op2(kind, x, y):  # into a buffer that no live intermediate occupies
                out, out_offs = pool[free.pop(0)]
                o, _, oo = wah.bitop_indexed_device(kind, x[0], x[1], y[0], y[1], n, scratch=scratch, out=out, out_offsets=out_offs, check=False)
                return o, oo

            def op_and_andnot(e, a, b):
                out, out_offs = pool[free.pop(0)]
                o, _, oo = wah.bitop_clauses_indexed_device([([e], False), ([a], False), ([b], True)], n, scratch=scratch, out=out,
                                                            out_offsets=out_offs, check=False)
                return o, oo

            def release(operand):
                free.append(slot_of[id(operand[0])])

            last["chain"], last["calls"] = chain(op2, op_and_andnot, slices_a, slices_b, ones, release)

        times = {"one call": [], "chain": []}
        for _ in range(REPS):
            times["one call"].append(step(f"one call, {k} slices", lambda: timed(one)))
            assert lib.wah_bsi_compare_status(scratch.data_ptr(), n, k, k, sp) == 0
            times["chain"].append(step(f"chain, {k} slices", lambda: timed(chained)))
            assert lib.wah_bitop_indexed_status(scratch.data_ptr(), n, sp) == 0

        def compare():
            one()
            torch.cuda.synchronize()
            words = int(last["one"][1].item())
            want, want_offs = res[:words].clone(), res_offs.clone()
            chained()
            torch.cuda.synchronize()
            o, oo = last["chain"]
            assert int(oo[n_seg].item()) == words and torch.equal(o[:words], want) and torch.equal(oo, want_offs), "RESULTS DIFFER"
            return words

        words = step(f"compare, {k} slices", compare)
        nbytes = 4 * row_words + 8 * n + 4 * words
        med = {w: statistics.median(ts) for w, ts in times.items()}
        say(f"{k:2d} and {k:2d} slices, uniform: one call {med['one call']:8.3f} ms ({min(times['one call']):.3f} .. {max(times['one call']):.3f})   "
            f"chain of {last['calls']:3d} calls {med['chain']:8.3f} ms ({min(times['chain']):.3f} .. {max(times['chain']):.3f})   "
            f"chain / one call {med['chain'] / med['one call']:.2f}   {nbytes / 1e6:.1f} MB -> {nbytes / (med['one call'] * 1e-3) / 8e12:.3f} of 8 TB/s   "
            f"result {words} words")
        del attr, bsi_a, bsi_b, slices_a, slices_b, pool
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

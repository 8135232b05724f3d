"""`lo <= value <= hi` over a bit-sliced attribute: the one call (columns.range_column -> wah_bsi_range_indexed_device) against the
only way to get the same answer without it -- the O'Neil & Quass sweep composed from the two-operand and eight-operand indexed
calls (wah_bitop_indexed_device, wah_bitop_many_indexed_device), every step of which writes a decoded bitmap and runs the compress
passes over it.  The composition is the cheapest one those calls allow (compose() below): one call per slice while the bounds'
bits agree, behind the first differing bit one call per side where the bound's bit keeps the side's rows equal (lo: 1, hi: 0)
and three where it moves rows inside (lo: 0, hi: 1), one three-operand OR at the end; capacities as lengths, no host round trip.

Attributes of 20 and 32 slices of 32 MiB each (uniform values: every slice is incompressible), a narrow range (about 2^-10 of the
width, the bounds share their top bits) and a wide one (about seven tenths of it).  Both ways are timed in turn, REPS times, each
time the mean over CALLS calls between two device events after a warm-up call (the one call as range_column makes it: the
slice table and the bounds are rewritten in place each time, which is part of what is timed); the table gives the median and min .. max -- the
spread a difference has to exceed -- and both ways must give the same words and the same index.  Beside the times: the bytes the
one call has to move, 4 x the slices' words read + 8 x n_words for the one decoded bitmap written and read by the compress passes,
and the fraction of 8 TB/s they give over the one call's median.  Every GPU step runs under a time limit of its own (a watchdog
thread ends the process when a step overruns it); everything runs in this one process.
usage: python tools/bsi_range_time.py [--out FILE.json] [--slices 20 32] [--segments 8457]"""
import argparse
import faulthandler
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, CALLS = 7, 3


def compose(op, slices, ones, n_bits, lo, hi, release=lambda x: None):
    """The sweep from binary steps: op(name, [operands]) -> operand with name in "and", "or", "andnot" (andnot: first AND NOT second;
    "or" takes up to three); release(operand): an intermediate the sweep no longer reads.  slices: most significant first; ones: the
    all-ones bitmap.  Returns (result, steps); None: all zeros."""
    top = (1 << n_bits) - 1
    if lo > hi or lo > top:
        return None, 0
    hi = min(hi, top)
    steps = 0
    eq_lo = eq_hi = ones
    inside = None
    diverged = False
    for i, b in enumerate(slices):
        sig = n_bits - 1 - i
        l, h = (lo >> sig) & 1, (hi >> sig) & 1
        if not diverged:
            before = eq_lo
            if l == h:
                eq_lo = eq_hi = op("and" if l else "andnot", [before, b])
                steps += 1
            else:  # l = 0, h = 1: the rows that follow lo and those that follow hi part
                eq_lo, eq_hi = op("andnot", [before, b]), op("and", [before, b])
                steps += 2
                diverged = True
            if before is not ones:
                release(before)
            continue
        for side in (0, 1):
            eq, bit = (eq_lo, l) if side == 0 else (eq_hi, h)
            if bit == side:  # lo's bit 0 / hi's bit 1: the rows that leave the bound go inside
                gone = op("and" if side == 0 else "andnot", [eq, b])
                steps += 1
                if inside is None:
                    inside = gone
                else:
                    grown = op("or", [inside, gone])
                    steps += 1
                    release(inside)
                    release(gone)
                    inside = grown
            kept = op("and" if bit else "andnot", [eq, b])
            steps += 1
            release(eq)
            if side == 0:
                eq_lo = kept
            else:
                eq_hi = kept
    if not diverged:
        return eq_lo, steps
    return op("or", [eq_lo, eq_hi] + ([inside] if inside is not None else [])), steps + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bsi_range_time.json"))
    ap.add_argument("--slices", type=int, nargs="*", default=[20, 32])
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
    rows = []
    print(f"{lib.wah_version().decode()}  slices of {n} words ({n * 4 / 2**20:.1f} MiB); median (min .. max) over {REPS} repetitions of "
          f"{CALLS} calls each, the two ways in turn", flush=True)
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
        slice_words = int(stream.numel())
        # the composition's operands: every slice as a stream and an index of its own, and all ones
        starts = seg_offsets[::segs].cpu().tolist()
        slices = [(stream[starts[i]: starts[i + 1]].clone(), (seg_offsets[i * segs: (i + 1) * segs + 1] - starts[i]).clone()) for i in range(k)]

        def all_ones():
            comp = wah.DeviceCompressor(n, device=dev, indexed=True)
            comp.run(torch.full((n,), -1, dtype=torch.int32, device=dev))
            return comp.result().clone(), comp.seg_offsets.clone()

        ones = step("all ones", all_ones)
        pool = [(torch.empty(cap, dtype=torch.int32, device=dev), torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)) for _ in range(8)]
        slot_of = {id(out): i for i, (out, _) in enumerate(pool)}
        table = torch.empty((k, 3), dtype=torch.int64, device=dev)
        bounds = torch.empty(2, dtype=torch.int64, device=dev)
        res = torch.empty(cap, dtype=torch.int32, device=dev)
        res_offs = torch.zeros(n_seg + 1, dtype=torch.int64, device=dev)
        top = (1 << k) - 1
        narrow_lo = (top // 2) ^ 0x2A5
        for name, lo, hi in (("narrow", narrow_lo, narrow_lo + (top >> 10)), ("wide", top // 7, top - top // 5)):
            last = {}

            def one():  # (range_column as a caller has it: the slice table and the bounds are rewritten in place on every call)
                last["one"] = wah.columns.range_column(wah, bsi, lo, hi, table=table, bounds=bounds, scratch=scratch, out=res, out_offsets=res_offs, check=False)

            def composed():
                free = list(range(len(pool)))

                def op(kind, operands):  # into a buffer that no live intermediate occupies
                    out, out_offs = pool[free.pop(0)]
                    if len(operands) == 2:
                        (a, ao), (b, bo) = operands
                        o, _, oo = wah.bitop_indexed_device(kind, a, ao, b, bo, n, scratch=scratch, out=out, out_offsets=out_offs, check=False)
                    else:
                        o, _, oo = wah.bitop_many_indexed_device(kind, operands, n, scratch=scratch, out=out, out_offsets=out_offs, check=False)
                    return o, oo

                def release(operand):
                    free.append(slot_of[id(operand[0])])

                last["composed"], last["steps"] = compose(op, slices, ones, k, lo, hi, release)

            times = {"one call": [], "composition": []}
            for _ in range(REPS):
                times["one call"].append(step(f"one call, {k} slices, {name}", lambda: timed(one)))
                assert lib.wah_bsi_range_status(scratch.data_ptr(), n, k, sp) == 0
                times["composition"].append(step(f"composition, {k} slices, {name}", lambda: timed(composed)))
                assert lib.wah_bitop_indexed_status(scratch.data_ptr(), n, sp) == 0

            def compare():
                one()
                torch.cuda.synchronize()
                words = int(last["one"][1].item())
                want, want_offs = res[:words].clone(), res_offs.clone()
                composed()
                torch.cuda.synchronize()
                o, oo = last["composed"]
                assert int(oo[n_seg].item()) == words and torch.equal(o[:words], want) and torch.equal(oo, want_offs), "RESULTS DIFFER"
                return words

            words = step(f"compare, {k} slices, {name}", compare)
            nbytes = 4 * slice_words + 8 * n
            med = {w: statistics.median(ts) for w, ts in times.items()}
            row = dict(slices=k, range=name, lo=lo, hi=hi, n_words=n, slice_words=slice_words, result_words=words, bytes_moved=nbytes,
                       composition_calls=last["steps"], one_call_ms=med["one call"], one_call_min_ms=min(times["one call"]),
                       one_call_max_ms=max(times["one call"]), composition_ms=med["composition"], composition_min_ms=min(times["composition"]),
                       composition_max_ms=max(times["composition"]), ratio=med["composition"] / med["one call"],
                       fraction_of_8_TBps=nbytes / (med["one call"] * 1e-3) / 8e12)
            rows.append(row)
            print(f"{k:2d} slices, {name:6s} [{lo}, {hi}]: one call {med['one call']:8.3f} ms ({min(times['one call']):.3f} .. {max(times['one call']):.3f})   "
                  f"composition of {last['steps']:3d} calls {med['composition']:8.3f} ms ({min(times['composition']):.3f} .. {max(times['composition']):.3f})   "
                  f"ratio {row['ratio']:.2f}   {nbytes / 1e6:.1f} MB -> {row['fraction_of_8_TBps']:.3f} of 8 TB/s   result {words} words", flush=True)
        del stream, seg_offsets, slices, pool, bsi
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(version=lib.wah_version().decode(), reps=REPS, calls=CALLS, timed="device events around CALLS calls after one warm-up call",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

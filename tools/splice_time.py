"""Appending a batch of rows to an index: the one call (wah_splice_indexed_device through columns.append_rows, the batch's own
small index built first and counted in) against the only road there is without it, a script of existing calls that depends on the
index type --
  bit-sliced attribute       columns.values_at_rows of EVERY row, a torch.cat with the batch, a whole new columns.bsi_from_values;
  equality-encoded attribute api.positions_device once per value, the batch's rows sorted in behind them, a whole new
                             api.from_positions_device.
A 20-slice attribute and an equality-encoded attribute of 1000 values, each of about 2^24 rows; a batch of one segment's rows
(31 744) appended at a segment edge (528 segments of rows in the index), and a batch of 1000 rows appended to exactly 2^24 rows, in
the middle of a segment and of a group.  Both roads are timed in turn, REPS times, between two device events after a warm-up; the
table gives the median and min .. max, and both roads must give the same stream and the same index.  Every GPU step runs under a
time limit of its own (a watchdog thread ends the process when a step overruns it).

usage: python tools/splice_time.py [--out FILE.txt] [--values 1000] [--bits 20]"""
import argparse
import faulthandler
import importlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 3
SEG_BITS = 31744


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_time.txt"))
    ap.add_argument("--values", type=int, default=1000)
    ap.add_argument("--bits", type=int, default=20)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds a single GPU step may take")
    args = ap.parse_args()

    import torch

    wah = importlib.import_module("gpu-wah_amd")
    lib = wah.lib()
    cols = wah.columns
    dev = "cuda:0"

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
        got = run()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), got

    gen = torch.Generator(device=dev)
    gen.manual_seed(4321)
    shapes = (("31744 rows at a segment edge", 528 * SEG_BITS, SEG_BITS), ("1000 rows in mid-segment", 1 << 24, 1000))
    lines = [f"{lib.wah_version().decode()}  append a batch to an index: median (min .. max) over {REPS} repetitions, the two roads in turn, "
             f"device events around one call after one warm-up"]
    print(lines[0], flush=True)

    for name, rows, batch_rows in shapes:
        # ---- the bit-sliced attribute ----
        values = torch.randint(0, 1 << args.bits, (rows + batch_rows,), generator=gen, device=dev)
        index = step("build the bit-sliced index", lambda: cols.bsi_from_values(wah, values[:rows].contiguous(), args.bits), 300)
        batch = values[rows:].contiguous()
        every = torch.arange(rows, dtype=torch.int64, device=dev)

        def bsi_one_call():
            return cols.append_rows(wah, index, rows, cols.bsi_from_values(wah, batch, args.bits), batch_rows)

        def bsi_script():
            old, _ = cols.values_at_rows(wah, index, every)
            return cols.bsi_from_values(wah, torch.cat([old, batch]), args.bits)

        # ---- the equality-encoded attribute ----
        keys = torch.randint(0, args.values, (rows + batch_rows,), generator=gen, device=dev)
        eq = step("build the equality-encoded index", lambda: cols.index_from_keys(wah, keys[:rows].contiguous(), args.values), 300)
        key_batch = keys[rows:].contiguous()
        segs = eq[2] // 992
        batch_at = rows + torch.arange(batch_rows, dtype=torch.int64, device=dev)
        ids = torch.arange(args.values, dtype=torch.int64, device=dev)

        def eq_one_call():
            return cols.append_rows(wah, eq, rows, cols.index_from_keys(wah, key_batch, args.values), batch_rows)

        def eq_script():
            lists = [wah.positions_device(eq[0], eq[1][v * segs: (v + 1) * segs + 1], eq[2])[0] for v in range(args.values)]
            counts = torch.tensor([int(p.numel()) for p in lists], dtype=torch.int64, device=dev)
            at = torch.cat(lists + [batch_at])
            key = torch.cat([torch.repeat_interleave(ids, counts), key_batch])
            order = torch.sort(key, stable=True).indices  # (a value's old rows ascend and lie in front of its batch rows)
            ends = torch.bincount(key, minlength=args.values)[: args.values].cumsum(0)
            n = max(-(-((rows + batch_rows + 31) // 32) // 992), 1) * 992
            stream, offs = wah.from_positions_device(at[order].contiguous(), ends, n)
            return stream, offs, n

        for what, one, script in ((f"{args.bits} slices", bsi_one_call, bsi_script), (f"{args.values} values", eq_one_call, eq_script)):
            times = {"one": [], "script": []}
            for _ in range(REPS):
                t, got = step(f"one call, {what}, {name}", lambda: timed(one))
                times["one"].append(t)
                t, want = step(f"script, {what}, {name}", lambda: timed(script), 600)
                times["script"].append(t)
            same = got[2:] == want[2:] and got[0].numel() == want[0].numel() and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            assert same, ("RESULTS DIFFER", what, name)
            med = {k: statistics.median(v) for k, v in times.items()}
            line = (f"{what:12s} {rows} rows + {name:30s}: one call {med['one']:10.3f} ms ({min(times['one']):.3f} .. {max(times['one']):.3f})   "
                    f"script {med['script']:10.3f} ms ({min(times['script']):.3f} .. {max(times['script']):.3f})   script / one call "
                    f"{med['script'] / med['one']:.2f}   {got[0].numel()} words out")
            print(line, flush=True)
            lines.append(line)
        del index, eq, values, keys
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

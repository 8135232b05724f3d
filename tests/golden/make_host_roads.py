#!/usr/bin/env python3
"""Generate tests/golden/host_roads.json -- what the host side of the indexed device calls answers without a device.

    python tests/golden/make_host_roads.py PATH/TO/libwah_hip.so [OUTPUT.json]

The file records ONE build of the library (the commit before the host roads were gathered into shared pieces) and is not
regenerated from a later tree: tests/test_host_roads_golden.py replays it against the library it is given.  Three parts:

  sizes     every sizing function a scratch layout feeds, over a grid that sits on the layouts' edges.  Per function the
            axes and the values in itertools.product order.
  refusals  per *_device entry point: calls with made-up, never-followed integers as device pointers, the return code and
            the wah_last_error() text of each.  One call per refuse() statement of the function (and per further way to trip
            it), and one per pair of consecutive statements that trips both, which pins their order.  EVERY call passes a
            scratch of 0 bytes or of one byte less than it needs: whatever is judged wrongly in front of it, the call ends
            at "scratch too small", never at a launch.
  statuses  every *_status function that judges its scratch pointer, called with a null one.

An argument is an integer, null, {"u8": [...]} or {"u64": [...]}: the last two are arrays in HOST memory (the attribute widths
of the grouped sum, the operand arrays of the eight-operand call), which the library reads before it judges the scratch.
"""
import ctypes
import importlib
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
WAH_ERR_ARG, WAH_ERR_WORKSPACE = -1, -2

K = 992 * 4096
N_WORDS = (0, 1, 991, 992, 993, 992 * 4095, K, K + 1, K * 4096, K * 4096 + 992, ((1 << 40) - 1) // 992 * 992, 1 << 40)
SLICES = (0, 1, 4, 5, 63, 64, 65)
LISTS = (1, 2, 4095, 4096, 4097, 1 << 16, 1 << 24)
ROWS = (0, 1, 63, 64, 65, 1 << 20, 1 << 40, 1 << 41)
GROUPS_QUERIES = ((1, 1), (7, 3), (64, 64), (4096, 1), (4097, 1), (64, 65))
FLAGS = (0, 1, 2, 3)

# function -> axes; an axis of pairs (GROUPS_QUERIES) is two arguments
SIZES = {
    "wah_bitop_indexed_scratch_bytes": (N_WORDS,),
    "wah_bitop_list_scratch_bytes": (N_WORDS, LISTS),
    "wah_bitop_clauses_scratch_bytes": (N_WORDS, LISTS, (1, 2, 4097)),
    "wah_bsi_range_scratch_bytes": (N_WORDS, SLICES),
    "wah_bsi_compare_scratch_bytes": (N_WORDS, SLICES, SLICES),
    "wah_bsi_kth_scratch_bytes": (N_WORDS, SLICES),
    "wah_bsi_kth_grouped_scratch_bytes": ((0, 992, K + 1, 1 << 40), SLICES, GROUPS_QUERIES),
    "wah_fetch_scratch_bytes": (N_WORDS, ROWS),
    "wah_select_scratch_bytes": (N_WORDS, (1, 2, 1 << 24)),
    "wah_from_positions_scratch_bytes": (N_WORDS, LISTS),
    "wah_from_positions_max_words": (N_WORDS, LISTS, ROWS),
    "wah_splice_scratch_bytes": (N_WORDS, LISTS, LISTS),
    "wah_splice_max_words": (N_WORDS, LISTS, (1, 2, 1 << 16), ROWS),
    "wah_bsi_build_scratch_bytes": (N_WORDS, SLICES),
    "wah_bsi_arith_scratch_bytes": (N_WORDS, SLICES, FLAGS),
    "wah_bsi_mul_scratch_bytes": (N_WORDS, (1, 20, 64), SLICES, FLAGS),
}


def flat(point):
    out = []
    for v in point:
        out.extend(v) if isinstance(v, tuple) else out.append(v)
    return out


# The refusals.  Per entry point: its arguments in the order of include/wah.h with a call that only its scratch size keeps from
# running, the sizing function and the arguments it takes, and per refuse() statement of the function, in the function's order,
# the ways to trip it (each a dict of overrides).  The first way of a statement, merged with the first way of the next, is the
# call that trips both.
T, T2, T3, OUT, WORDS, OFFS, SC = 0x20000, 0x28000, 0x2C000, 0x30000, 0x40000, 0x50000, 0x100000
STRICT_OUTPUT = [dict(out=None), dict(out=OUT + 2), dict(out_words=None), dict(out_words=WORDS + 4), dict(out_offsets=None),
                 dict(out_offsets=OFFS + 4)]
WEAK_OUTPUT = [dict(out_words=None), dict(out=None)]
BAD_SCRATCH = [dict(scratch=None), dict(scratch=SC + 128)]
BAD_TABLE = [dict(n_operands=0), dict(n_operands=(1 << 24) + 1), dict(table=None), dict(table=T + 4), dict(n_words=1 << 40)]
TAIL = dict(out=OUT, cap=1000, out_words=WORDS, out_offsets=OFFS, scratch=SC, scratch_bytes=0, stream=None)
WIDTHS = {"u8": [3, 2] + [1] * 78}

REFUSALS = {
    "wah_bitop_indexed_device": dict(
        base=dict(op=1, n_words=992 * 4, a=0x10000, a_words=10, a_offs=0x11000, b=0x12000, b_words=12, b_offs=0x13000, **TAIL),
        size=("wah_bitop_indexed_scratch_bytes", ("n_words",)),
        faults=[[dict(op=4), dict(op=-1)] + BAD_SCRATCH,
                [dict(a_offs=None), dict(b_offs=None), dict(a=None), dict(b=None), dict(n_words=1 << 40), dict(a_words=1 << 40),
                 dict(b_words=1 << 40), dict(a=0x10002), dict(b=0x12002)]]),
    "wah_bitop_many_indexed_device": dict(
        base=dict(op=1, n_words=992 * 4, n_operands=3, streams={"u64": [0x10000, 0x12000, 0x14000] + [0x16000] * 6},
                  stream_words={"u64": [10, 12, 14] + [1] * 6}, offsets={"u64": [0x11000, 0x13000, 0x15000] + [0x17000] * 6}, **TAIL),
        size=("wah_bitop_indexed_scratch_bytes", ("n_words",)),
        faults=[[dict(op=4)] + BAD_SCRATCH,
                [dict(n_operands=0), dict(n_operands=9), dict(streams=None), dict(stream_words=None), dict(offsets=None), dict(n_words=1 << 40)],
                [dict(offsets={"u64": [0x11000, 0, 0x15000] + [0x17000] * 6}), dict(streams={"u64": [0x10000, 0x12000, 0] + [0x16000] * 6}),
                 dict(stream_words={"u64": [1 << 40, 12, 14] + [1] * 6}), dict(streams={"u64": [0x10002, 0x12000, 0x14000] + [0x16000] * 6})]]),
    "wah_bitop_list_indexed_device": dict(
        base=dict(op=0, n_words=992 * 4, n_operands=5, table=T, **TAIL),
        size=("wah_bitop_list_scratch_bytes", ("n_words", "n_operands")),
        faults=[[dict(op=4)] + BAD_SCRATCH, BAD_TABLE, WEAK_OUTPUT]),
    "wah_bitop_clauses_indexed_device": dict(
        base=dict(n_words=992 * 4, n_clauses=2, clause_ends=T2, n_operands=5, table=T, **TAIL),
        size=("wah_bitop_clauses_scratch_bytes", ("n_words", "n_operands", "n_clauses")),
        faults=[BAD_SCRATCH, BAD_TABLE, [dict(n_clauses=0), dict(n_clauses=6), dict(clause_ends=None), dict(clause_ends=T2 + 4)], WEAK_OUTPUT]),
    "wah_bsi_range_indexed_device": dict(
        base=dict(n_words=992 * 4, n_slices=20, table=T, bounds=T2, flags=1, **TAIL),
        size=("wah_bsi_range_scratch_bytes", ("n_words", "n_slices")),
        faults=[[dict(n_slices=0), dict(n_slices=65), dict(flags=2)],
                [dict(table=None), dict(table=T + 4), dict(bounds=None), dict(bounds=T2 + 4)] + BAD_SCRATCH,
                WEAK_OUTPUT + [dict(n_words=1 << 40)]]),
    "wah_bsi_compare_indexed_device": dict(
        base=dict(op=0, n_words=992 * 4, n_slices_a=20, n_slices_b=7, table=T, flags=3, **TAIL),
        size=("wah_bsi_compare_scratch_bytes", ("n_words", "n_slices_a", "n_slices_b")),
        faults=[[dict(op=6), dict(op=-1)],
                [dict(n_slices_a=0), dict(n_slices_a=65), dict(n_slices_b=0), dict(n_slices_b=65), dict(flags=4)],
                [dict(table=None), dict(table=T + 4)] + BAD_SCRATCH,
                WEAK_OUTPUT + [dict(n_words=1 << 40)]]),
    "wah_bsi_kth_indexed_device": dict(
        base=dict(n_words=992 * 4, n_filters=2, n_slices=20, table=T, query=T2, result=T3, scratch=SC, scratch_bytes=0, stream=None),
        size=("wah_bsi_kth_scratch_bytes", ("n_words", "n_slices")),
        faults=[[dict(n_slices=0), dict(n_slices=65), dict(n_filters=65)],
                [dict(table=None), dict(table=T + 4), dict(query=None), dict(query=T2 + 4), dict(result=None), dict(result=T3 + 4)] + BAD_SCRATCH,
                [dict(n_words=1 << 40)]]),
    "wah_bsi_kth_grouped_indexed_device": dict(
        base=dict(n_words=992 * 4, n_filters=2, filters=T, n_groups=7, rows_per_group=2, groups=T2, n_slices=20, slices=T3, n_queries=3,
                  queries=0x60000, results=0x70000, scratch=SC, scratch_bytes=0, stream=None),
        size=("wah_bsi_kth_grouped_scratch_bytes", ("n_words", "n_slices", "n_groups", "n_queries")),
        faults=[[dict(n_slices=0), dict(n_slices=65), dict(n_filters=65)],
                [dict(rows_per_group=0), dict(rows_per_group=9), dict(n_groups=0), dict(n_groups=4097), dict(n_queries=0), dict(n_queries=4097),
                 dict(n_groups=64, n_queries=65)],
                [dict(filters=None), dict(filters=T + 4), dict(groups=None), dict(groups=T2 + 4), dict(slices=None), dict(slices=T3 + 4)],
                [dict(queries=None), dict(queries=0x60004), dict(results=None), dict(results=0x70004)] + BAD_SCRATCH,
                [dict(n_words=1 << 40)]]),
    "wah_fetch_indexed_device": dict(
        base=dict(mode=0, n_words=992 * 3, n_operands=20, table=T, rows=T2, n_rows=1000, out=OUT, scratch=SC, scratch_bytes=0, stream=None),
        size=("wah_fetch_scratch_bytes", ("n_words", "n_rows")),
        faults=[[dict(mode=2)], [dict(n_operands=0), dict(n_operands=65), dict(mode=1, n_operands=(1 << 24) + 1)], [dict(n_words=0)],
                [dict(n_rows=1 << 40), dict(n_words=1 << 40)],
                [dict(table=None), dict(table=T + 4), dict(rows=None), dict(rows=T2 + 4), dict(out=None), dict(out=OUT + 4)] + BAD_SCRATCH]),
    "wah_count_list_indexed_device": dict(
        base=dict(n_words=992 * 4, n_operands=5, table=T, counts=T2, scratch=SC, scratch_bytes=0, stream=None),
        size=("wah_select_scratch_bytes", ("n_words", "n_operands")),
        faults=[BAD_SCRATCH, BAD_TABLE, [dict(counts=None), dict(counts=T2 + 4)]]),
    "wah_count_masked_indexed_device": dict(
        base=dict(n_words=992 * 4, n_masks=3, masks=T3, n_operands=5, table=T, counts=T2, scratch=SC, scratch_bytes=0, stream=None),
        size=("wah_select_scratch_bytes", ("n_words", "n_operands")),
        faults=[BAD_SCRATCH,
                [dict(n_masks=0), dict(n_operands=0), dict(n_masks=1 << 12, n_operands=(1 << 12) + 1), dict(masks=None), dict(masks=T3 + 4),
                 dict(table=None), dict(table=T + 4), dict(n_words=1 << 40)],
                [dict(counts=None), dict(counts=T2 + 4)]]),
    "wah_group_sum_indexed_device": dict(
        base=dict(n_words=992 * 4, n_filters=2, filters=T3, n_groups=4, rows_per_group=2, groups=T2, n_operands=5, table=T, n_attrs=2,
                  attr_bits=WIDTHS, group_rows=0x60000, counts=0x70000, sums=0x80000, scratch=SC, scratch_bytes=0, stream=None),
        size=("wah_select_scratch_bytes", ("n_words", "n_operands")),
        faults=[BAD_SCRATCH,
                [dict(n_filters=65), dict(filters=None), dict(filters=T3 + 4)],
                [dict(rows_per_group=0), dict(rows_per_group=9), dict(n_groups=0), dict(n_groups=(1 << 24) + 1), dict(groups=None),
                 dict(groups=T2 + 4), dict(table=None), dict(table=T + 4), dict(n_words=1 << 40)],
                [dict(n_attrs=65), dict(n_attrs=0), dict(attr_bits=None)],
                [dict(attr_bits={"u8": [0, 5] + [1] * 78}), dict(attr_bits={"u8": [3, 65] + [1] * 78})],
                [dict(n_operands=7)],
                [dict(sums=None), dict(sums=0x80004), dict(group_rows=None), dict(group_rows=0x60004), dict(counts=None), dict(counts=0x70004)]]),
    "wah_positions_indexed_device": dict(
        base=dict(n_words=992 * 4, stream_=0x10000, stream_words=10, offsets=0x11000, first_rank=0, out=OUT, cap=100, info=WORDS, scratch=SC,
                  scratch_bytes=0, stream=None),
        size=("wah_select_scratch_bytes", ("n_words", "stream_words")),
        faults=[BAD_SCRATCH, [dict(n_words=1 << 40)], [dict(info=None), dict(info=WORDS + 4), dict(out=None), dict(out=OUT + 4)]]),
    "wah_from_positions_device": dict(
        base=dict(n_words=992 * 4, n_lists=5, list_ends=T, rows=T2, n_rows=100, **TAIL),
        size=("wah_from_positions_scratch_bytes", ("n_words", "n_lists")),
        faults=[[dict(n_rows=1 << 40), dict(n_lists=0), dict(n_lists=(1 << 24) + 1), dict(n_words=0), dict(n_words=1 << 40)],
                [dict(n_lists=1 << 21, n_words=992 * 1024), dict(n_lists=2, n_words=992 << 30)],
                BAD_SCRATCH, [dict(list_ends=None), dict(list_ends=T + 4), dict(rows=None), dict(rows=T2 + 4)], STRICT_OUTPUT]),
    "wah_splice_indexed_device": dict(
        base=dict(n_words=992 * 4, n_columns=3, n_pieces=2, pieces=T2, table=T, **TAIL),
        size=("wah_splice_scratch_bytes", ("n_words", "n_columns", "n_pieces")),
        faults=[[dict(n_pieces=0), dict(n_pieces=(1 << 16) + 1), dict(n_columns=0), dict(n_columns=(1 << 24) + 1), dict(n_pieces=1 << 16, n_columns=257),
                 dict(n_words=0), dict(n_words=1 << 40)],
                [dict(n_columns=1 << 21, n_words=992 * 1024), dict(n_columns=2, n_words=992 << 30)],
                BAD_SCRATCH, [dict(pieces=None), dict(pieces=T2 + 4), dict(table=None), dict(table=T + 4)], STRICT_OUTPUT]),
    "wah_bsi_build_device": dict(
        base=dict(n_words=992 * 4, n_bits=20, values=T, n_rows=1000, exists=None, **TAIL),
        size=("wah_bsi_build_scratch_bytes", ("n_words", "n_bits")),
        faults=[[dict(n_bits=0), dict(n_bits=65)],
                [dict(n_words=993), dict(n_words=0), dict(n_words=1 << 40), dict(n_words=992 << 25, n_bits=64)],
                [dict(n_rows=1 << 50)], [dict(values=None), dict(values=T + 4)], STRICT_OUTPUT, BAD_SCRATCH]),
    "wah_bsi_arith_indexed_device": dict(
        base=dict(op=0, n_words=992 * 4, n_slices_a=20, n_slices_b=7, n_slices_out=21, table=T, flags=3, **TAIL),
        size=("wah_bsi_arith_scratch_bytes", ("n_words", "n_slices_out", "flags")),
        faults=[[dict(op=2), dict(op=-1)],
                [dict(n_slices_a=0), dict(n_slices_a=65), dict(n_slices_b=0), dict(n_slices_b=65), dict(n_slices_out=0), dict(n_slices_out=65),
                 dict(flags=4)],
                [dict(n_words=993), dict(n_words=0), dict(n_words=1 << 40), dict(n_words=992 << 25, n_slices_out=64)],
                [dict(table=None), dict(table=T + 4)] + BAD_SCRATCH, STRICT_OUTPUT]),
    "wah_bsi_mul_indexed_device": dict(
        base=dict(n_words=992 * 4, n_slices_a=20, n_slices_b=7, n_slices_out=27, table=T, flags=3, **TAIL),
        size=("wah_bsi_mul_scratch_bytes", ("n_words", "n_slices_a", "n_slices_out", "flags")),
        faults=[[dict(n_slices_a=0), dict(n_slices_a=65), dict(n_slices_b=0), dict(n_slices_b=65), dict(n_slices_out=0), dict(n_slices_out=65),
                 dict(flags=4)],
                [dict(n_words=993), dict(n_words=0), dict(n_words=1 << 40), dict(n_words=992 << 25, n_slices_out=64)],
                [dict(table=None), dict(table=T + 4)] + BAD_SCRATCH, STRICT_OUTPUT]),
}

STATUSES = {
    "wah_bitop_status": (None, 992, 10, 12, None),
    "wah_bitop_indexed_status": (None, 992, None),
    "wah_bitop_list_status": (None, 992, 5, None),
    "wah_bitop_clauses_status": (None, 992, 5, 2, None),
    "wah_bsi_range_status": (None, 992, 20, None),
    "wah_bsi_compare_status": (None, 992, 20, 7, None),
    "wah_bsi_arith_status": (None, 992, 21, 3, None),
    "wah_bsi_mul_status": (None, 992, 20, 27, 3, None),
    "wah_bsi_kth_status": (None, None),
    "wah_bsi_kth_grouped_status": (None, None),
    "wah_fetch_status": (None, None),
    "wah_select_status": (None, None),
    "wah_from_positions_status": (None, None),
    "wah_splice_status": (None, None),
    "wah_bsi_build_status": (None, 992, 21, None),
}


def native(arg):
    """A recorded argument as ctypes takes it; a host array is kept alive by the caller's list."""
    if isinstance(arg, dict):
        (kind, values), = arg.items()
        ctype = {"u8": ctypes.c_uint8, "u64": ctypes.c_uint64}[kind]
        return ctypes.cast((ctype * len(values))(*values), ctypes.c_void_p)
    return arg


def refusal_calls(spec):
    """The calls a function's entry records, as (arguments by name, short): the call that only its scratch keeps from running, every
    way to trip every statement, every consecutive pair.  short: the scratch is one byte less than the call needs, not 0 bytes."""
    base, faults = spec["base"], spec["faults"]
    calls = [(dict(base), False), (dict(base), True)]
    for ways in faults:
        calls += [(dict(base, **w), False) for w in ways]
    for a, b in zip(faults, faults[1:]):
        calls.append((dict(base, **a[0], **b[0]), False))
    calls.append((dict(base, **faults[-1][0]), True))
    return calls


def main():
    lib_path = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "host_roads.json")
    os.environ["WAH_LIB_PATH"] = lib_path
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("gpu-wah_amd")
    assert os.path.samefile(pkg.lib_path(), lib_path)
    lib = pkg.lib()

    sizes = {}
    for name, axes in SIZES.items():
        fn = getattr(lib, name)
        sizes[name] = {"axes": [[list(v) if isinstance(v, tuple) else v for v in axis] for axis in axes],
                       "values": [int(fn(*flat(p))) for p in itertools.product(*axes)]}

    refusals = {}
    for name, spec in REFUSALS.items():
        fn = getattr(lib, name)
        size_fn, size_args = spec["size"]
        need = int(getattr(lib, size_fn)(*[spec["base"][k] for k in size_args]))
        calls = []
        for named, short in refusal_calls(spec):
            named["scratch_bytes"] = need - 1 if short else 0
            args = list(named.values())
            keep = [native(a) for a in args]
            rc = int(fn(*keep))
            text = lib.wah_last_error().decode()
            if rc not in (WAH_ERR_ARG, WAH_ERR_WORKSPACE):
                raise SystemExit(f"{name}{tuple(args)} returned {rc} ({text!r}): not a refusal, nothing written")
            calls.append({"args": args, "rc": rc, "error": text})
        refusals[name] = calls

    statuses = {}
    for name, args in STATUSES.items():
        rc = int(getattr(lib, name)(*args))
        if rc != WAH_ERR_ARG:
            raise SystemExit(f"{name} with a null scratch returned {rc}")
        statuses[name] = {"args": list(args), "rc": rc}

    with open(out_path, "w") as f:
        json.dump({"sizes": sizes, "refusals": refusals, "statuses": statuses}, f, separators=(",", ":"))
        f.write("\n")
    n_calls = sum(len(c) for c in refusals.values())
    print(f"{out_path}: {sum(len(s['values']) for s in sizes.values())} sizes, {n_calls} refusals, {len(statuses)} statuses, "
          f"{os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()

"""Grouped SUM / COUNT under a filter: ONE wah_group_sum_indexed_device call (api.group_sum_device over ready tables, check=False;
the sums then read back and joined to Python ints) against the only road there was before it: per group one
columns.filter_columns (the filter AND the group's rows, one compressed bitmap and index written per group, check=False), one
api.count_masked_device over all slices with those G results as the masks, the counts read back and folded in Python.  2^24 rows,
keys of 3 x 2 values (uniform), a filter that selects about 98 % of the rows and one that selects about 1 % (a range over a
uniform 20-bit attribute), one attribute of 20 bits and four of 8 + 20 + 20 + 40 (uniform random values: every slice is
incompressible).  Both roads in one process, REPS times in turn after a warm-up, device events around each (the read-back and
the fold are inside them on both roads); every time and min .. max are printed -- the spread a difference has to exceed -- and
both roads must give the same rows and sums.  No ratio is expected in advance: what comes out is written down.
usage: python tools/group_sum_time.py [output file]    (default: profiles/group_sum_time.txt)"""
import importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
wah = importlib.import_module("gpu-wah_amd")
lib = wah.lib()
DEV = "cuda:0"
ROWS = 1 << 24
KEYS = (3, 2)
FILTERS = (("about 98 %", 0.98), ("about  1 %", 0.01))
ATTRIBUTES = ((20,), (8, 20, 20, 40))
REPS = 5
U64 = (1 << 64) - 1

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "group_sum_time.txt")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(run):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    result = run()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]), result


def spread(ts):
    return f"{min(ts):9.3f} .. {max(ts):9.3f}"


def every(ts):
    return " ".join(f"{t:.3f}" for t in ts)


def verdict(new, base):
    if max(new) < min(base):
        return f"one call faster, {min(base) / max(new):.1f}x at the least"
    if min(new) > max(base):
        return f"one call SLOWER, {min(new) / max(base):.1f}x at the least"
    return "within the spread"


def uniform(gen, n_bits):
    wide = (torch.randint(0, 1 << 32, (ROWS,), dtype=torch.int64, device=DEV, generator=gen) << 31) | torch.randint(0, 1 << 31, (ROWS,), dtype=torch.int64, device=DEV, generator=gen)
    return wide >> (63 - n_bits)  # uniform over [0, 2^n_bits): every slice is incompressible


gen = torch.Generator(device=DEV).manual_seed(6161)
N = -(-(ROWS // 32) // 992) * 992
keys = [wah.columns.index_from_keys(wah, torch.randint(0, k, (ROWS,), dtype=torch.int64, device=DEV, generator=gen), k, n_words_per_column=N) for k in KEYS]
steer = wah.columns.bsi_from_values(wah, uniform(gen, 20), 20, n_words_per_column=N)
pool = {bits: wah.columns.bsi_from_values(wah, uniform(gen, bits), bits, n_words_per_column=N) for bits in (8, 20, 40)}
second_20 = wah.columns.bsi_from_values(wah, uniform(gen, 20), 20, n_words_per_column=N)
G = KEYS[0] * KEYS[1]


def row(filter_name, share, widths):
    where = wah.columns.range_column(wah, steer, 0, int(share * (1 << 20)) - 1)
    attributes, seen_20 = [], False
    for bits in widths:
        attributes.append(second_20 if bits == 20 and seen_20 else pool[bits])
        seen_20 |= bits == 20
    slices = torch.cat([wah.columns.column_operand_table(a[0], a[1], N, list(range(a[3]))) for a in attributes])
    k = int(slices.shape[0])
    filters = wah.bitop_operand_table([where])
    key_tables = [wah.columns.column_operand_table(st, offs, N, list(range(v))) for (st, offs, _), v in zip(keys, KEYS)]
    picks = torch.cartesian_prod(*[torch.arange(v, device=DEV) for v in KEYS])
    groups = torch.stack([t[picks[:, r]] for r, t in enumerate(key_tables)], dim=1).contiguous().view(-1, 3)
    scratch = torch.empty(int(lib.wah_select_scratch_bytes(N, k)), dtype=torch.uint8, device=DEV)
    outs = dict(group_rows=torch.empty(G, dtype=torch.int64, device=DEV), counts=torch.empty((G, k), dtype=torch.int64, device=DEV),
                sums=torch.empty((G, len(widths), 2), dtype=torch.int64, device=DEV))

    def new():
        rows, _, sums = wah.group_sum_device(filters, groups, slices, list(widths), N, rows_per_group=len(KEYS), scratch=scratch, check=False, **outs)
        words = sums.tolist()
        return rows.tolist(), [[(low & U64) + ((high & U64) << 64) for low, high in group] for group in words]

    filter_scratch = [torch.empty(int(lib.wah_bitop_clauses_scratch_bytes(N, 3, 3)), dtype=torch.uint8, device=DEV) for _ in range(G)]
    filter_tables = [(torch.empty((3, 3), dtype=torch.int64, device=DEV), torch.empty(3, dtype=torch.int64, device=DEV)) for _ in range(G)]
    masks = torch.empty((G, 3), dtype=torch.int64, device=DEV)
    base_counts = torch.empty((G, k), dtype=torch.int64, device=DEV)
    base_rows = torch.empty(G, dtype=torch.int64, device=DEV)

    def base(with_rows=False):
        kept = []
        for g in range(G):
            i, j = divmod(g, KEYS[1])
            predicates = [(where[0], where[1], [0], False), (keys[0][0], keys[0][1], [i], False), (keys[1][0], keys[1][1], [j], False)]
            out, _, out_offsets = wah.columns.filter_columns(wah, predicates, N, tables=filter_tables[g], scratch=filter_scratch[g], check=False)
            kept.append((out, out_offsets))
            masks[g] = torch.tensor([out.data_ptr(), out.numel(), out_offsets.data_ptr()], dtype=torch.int64)
        counts = wah.count_masked_device(masks, slices, N, scratch=scratch, counts=base_counts, check=False).tolist()
        # (COUNT(*) per group would be one more call on this road; it is made for the comparison of the results only, not timed)
        rows = wah.count_device(masks, N, scratch=scratch, counts=base_rows, check=False).tolist() if with_rows else None
        sums, at = [[] for _ in range(G)], 0
        for bits in widths:
            for g in range(G):
                sums[g].append(sum(int(c) << (bits - 1 - s) for s, c in enumerate(counts[g][at: at + bits])))
            at += bits
        return rows, sums

    got, want = new(), base(with_rows=True)  # warm-up
    torch.cuda.synchronize()
    assert lib.wah_select_status(scratch.data_ptr(), None) == 0
    assert got == want, "THE TWO ROADS DIFFER"
    t_new, t_base = [], []
    for _ in range(REPS):
        t_new.append(timed(new)[0])
        t_base.append(timed(base)[0])
    selected = sum(got[0])
    say(f"filter selects {filter_name} ({selected} of {ROWS} rows)  {G} groups  attributes of {' + '.join(str(b) for b in widths)} bits ({k} slices of {N} words)")
    say(f"    one call                                         {spread(t_new)} ms   ({every(t_new)})")
    say(f"    {G} filter_columns, one count_masked, Python fold   {spread(t_base)} ms   ({every(t_base)})")
    say(f"    {verdict(t_new, t_base)}")


say(f"{lib.wah_version().decode()}  min .. max over {REPS} repetitions in turn after a warm-up, device events around each road; uniform random keys and values")
for filter_name, share in FILTERS:
    for widths in ATTRIBUTES:
        row(filter_name, share, widths)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")

"""Shared helpers of the membership tests (wah_bsi_member_indexed_device, include/wah.h): a numpy model that answers `value IN (set)`
from the VALUES, the kernel's steps restated in numpy from the SLICES, seven wrong models of that restatement, and the builders
of the named cases.  A bitmap of n_words words has 32 * n_words rows, row p at word p // 32, bit p % 32; values and list entries are
numpy uint64, a bit array is uint32 words.

A case is a dict: n (words), k (slices), values, exists (or None), negate, and either
  members (uint64 [capacity]), count (int, or None: the capacity)                 -- a sorted list
  words (uint32 [ceil(set_bits / 32)]), set_bits                                  -- a bit array."""
import numpy as np

from tests import _bsi

U64_MAX = _bsi.U64_MAX
M31 = np.uint32(0x7FFFFFFF)
SEG_WORDS, SEG_GROUPS, SEG_BITS = 992, 1024, 31 * 1024
HALF_GROUPS, HALF_ROWS, HALF_WORDS = 512, 31 * 512, 496
WRONG = ("last entry never compared", "capacity for the count", "spare bits honoured", "negate without existence", "cut to 32 bits",
         "modulo the width", "second half over the first")


def is_bitset(case):
    return "words" in case


# ---- the value model -------------------------------------------------------------------------------------------------------------
def expected(case):
    """The model: the rows whose value is in the set (NEGATE: is not) that exist -- np.isin on the values, never on slices.  Rows
    the caller does not have are rows of value 0 like any other."""
    v = case["values"]
    if is_bitset(case):
        inside = v < np.uint64(case["set_bits"])
        match = np.zeros(v.shape, bool)
        at = v[inside]
        match[inside] = (case["words"][(at >> np.uint64(5)).astype(np.int64)] >> (at & np.uint64(31)).astype(np.uint32)) & np.uint32(1) != 0
    else:
        count = case["members"].size if case["count"] is None else case["count"]
        match = np.isin(v, case["members"][:count])
    if case["negate"]:
        match = ~match
    return _bsi.pack_bits(match if case["exists"] is None else match & case["exists"])


# ---- the kernel's steps ------------------------------------------------------------------------------------------------------------
def search(members, count, v, wrong=None):
    """The branch-free search written out: base is the last entry <= v among those looked at (or 0); count steps are the same
    for every row.  Returns the rows' matches."""
    if wrong == "last entry never compared" and count:
        count -= 1
    base = np.zeros(v.shape, np.int64)
    n = count
    while n > 1:
        half = n >> 1
        base += np.where(members[base + half] <= v, half, 0)
        n -= half
    if count == 0:
        return np.zeros(v.shape, bool)
    return members[base] == v


def kernel(case, wrong=None):
    """wah_member.hip restated: the items (a segment, above 32 slices a segment and a half of its groups), the values out of the
    item's slices, the probe, the 31-bit groups with NEGATE and the existence group, groups at and behind nvalid zero, and the
    item's words -- 992, or the 496 of its half."""
    n, k, negate = case["n"], case["k"], case["negate"]
    slices = _bsi.build_slices(case["values"], k, case["exists"])
    groups = (32 * n + 30) // 31
    n_seg = -(-groups // SEG_GROUPS)
    out_words = (31 * groups + 31) // 32
    padded = np.zeros((slices.shape[0], n_seg * SEG_WORDS), np.uint32)
    padded[:, :n] = slices
    out = np.zeros(n_seg * SEG_WORDS, np.uint32)
    wide = k > 32
    halves = 2 if wide else 1
    item_groups = HALF_GROUPS if wide else SEG_GROUPS
    for t in range(n_seg * halves):
        seg, half = divmod(t, halves)
        nvalid = min(groups - seg * SEG_GROUPS, SEG_GROUPS)
        first = seg * SEG_BITS + half * HALF_ROWS
        bits = np.stack([_bsi.unpack_bits(row[seg * SEG_WORDS: (seg + 1) * SEG_WORDS])[first - seg * SEG_BITS:][: 31 * item_groups] for row in padded])
        lo, hi = np.zeros(31 * item_groups, np.uint64), np.zeros(31 * item_groups, np.uint64)
        for i in range(k):  # the fold: one bit per row and slice, into the half of the value the slice belongs to
            sig = k - 1 - i
            if sig >= 32:
                hi |= bits[i].astype(np.uint64) << np.uint64(sig - 32)
            else:
                lo |= bits[i].astype(np.uint64) << np.uint64(sig)
        v = lo if wrong == "cut to 32 bits" else (hi << np.uint64(32)) | lo
        if is_bitset(case):
            limit = 32 * case["words"].size if wrong == "spare bits honoured" else case["set_bits"]
            inside = v < np.uint64(limit)
            match = np.zeros(v.shape, bool)
            at = v[inside]
            match[inside] = (case["words"][(at >> np.uint64(5)).astype(np.int64)] >> (at & np.uint64(31)).astype(np.uint32)) & np.uint32(1) != 0
        else:
            members = case["members"]
            count = members.size if case["count"] is None or wrong == "capacity for the count" else min(case["count"], members.size)
            if wrong == "modulo the width" and k < 64:
                members = np.sort(members[:count] & np.uint64((1 << k) - 1))
            match = search(members, count, v, wrong)
        word = (match.reshape(item_groups, 31).astype(np.uint32) << np.arange(31, dtype=np.uint32)).sum(axis=1, dtype=np.uint32)
        if negate:
            word ^= M31
        if case["exists"] is not None and not (wrong == "negate without existence" and negate):
            have = bits[k].reshape(item_groups, 31).astype(np.uint32) << np.arange(31, dtype=np.uint32)
            word &= have.sum(axis=1, dtype=np.uint32)
        g = half * HALF_GROUPS + np.arange(item_groups)
        word[g >= nvalid] = 0
        # the store: 31 -> 32 repack of the item's groups into the words it owns
        rows = ((word[:, None] >> np.arange(31, dtype=np.uint32)) & np.uint32(1)).astype(bool).reshape(-1)
        at = seg * SEG_WORDS + (0 if wrong == "second half over the first" else half * HALF_WORDS)
        out[at: at + rows.size // 32] = _bsi.pack_bits(rows)
    out[out_words:] = 0
    return out[:n]


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def sorted_set(entries):
    return np.sort(np.array([int(e) for e in entries], dtype=np.uint64))


def list_case(n, k, values, exists, entries, negate=False, count=None, poison=()):
    """A list: `entries` sorted, then `poison` behind the count (the count is then len(entries))."""
    members = sorted_set(entries)
    if len(poison):
        count = members.size
        members = np.concatenate([members, np.array([int(p) for p in poison], dtype=np.uint64)])
    return dict(n=n, k=k, values=values, exists=exists, negate=negate, members=members, count=count)


def bitset_case(n, k, values, exists, set_bits, rng, negate=False, spare_ones=True, density=0.5):
    words = _bsi.pack_bits(rng.random(32 * ((set_bits + 31) // 32)) < density) if set_bits else np.zeros(0, np.uint32)
    if set_bits % 32 and spare_ones:
        words[-1] |= np.uint32((0xFFFFFFFF << (set_bits % 32)) & 0xFFFFFFFF)  # the last word's spare bits: never looked at
    return dict(n=n, k=k, values=values, exists=exists, negate=negate, words=words, set_bits=set_bits)


def attribute(n, k, with_exists, seed=0, domain=None):
    """Uniform values over the width, or half of them below `domain`; an existence bitmap of density 0.9."""
    rng = np.random.default_rng(104729 * k + n + seed)
    rows = 32 * n
    values = _bsi.uniform_values(rng, rows, k)
    if domain is not None:
        small = rng.integers(0, max(domain, 1), rows, dtype=np.uint64)
        values = np.where(rng.random(rows) < 0.5, small, values)
    exists = rng.random(rows) < 0.9 if with_exists else None
    return values, exists, rng


def headline(n, k, with_exists, negate=False, bitset=False):
    """The headline case of a size and width: about a third of the present values in the set (the whole domain's for narrow
    widths), and as many absent ones."""
    top = (1 << k) - 1
    if bitset:
        set_bits = min(top + 1, (1 << 16) + 5)
        values, exists, rng = attribute(n, k, with_exists, 1, domain=min(set_bits + 40, top + 1))
        case = bitset_case(n, k, values, exists, set_bits, rng, negate)
        if set_bits <= 4:  # a domain of two or four values: one, two of them in the set
            case["words"][0] = (case["words"][0] & np.uint32(0xFFFFFFF0 | (0xF << set_bits) & 0xF)) | np.uint32(0b01 if set_bits == 2 else 0b0110)
        return case
    values, exists, rng = attribute(n, k, with_exists)
    present = np.unique(values)
    take = present[rng.random(present.size) < (0.34 if present.size > 2 else 0.5)][:400]
    if take.size == 0 or take.size == present.size:
        take = present[:1]
    absent = [int(v) ^ 1 for v in take[:50] if int(v) ^ 1 not in set(present.tolist())] if k > 8 else []
    return list_case(n, k, values, exists, list(take) + absent, negate)


def list_edges(k=20, n=SEG_WORDS + 5, with_exists=True):
    """name -> case: every edge the interface names for a list."""
    values, exists, rng = attribute(n, k, with_exists, 2)
    top = (1 << k) - 1
    have = np.unique(values if exists is None else values[exists])
    lo, hi, mid = int(have[0]), int(have[-1]), int(have[have.size // 2])
    everything = set(np.unique(values).tolist())
    sample = [int(v) for v in have[:: max(have.size // 1000, 1)]]
    cases = {}
    for count in (0, 1, 2, 63, 64, 65, 1000):
        cases[f"count {count}"] = list_case(n, k, values, exists, sample[:count])
        cases[f"count {count} poisoned"] = list_case(n, k, values, exists, sample[:count], poison=[hi, hi] + sample[count: count + 40])
    cases["duplicates"] = list_case(n, k, values, exists, [lo, lo, mid, mid, mid, hi, hi])
    cases["smallest and largest present"] = list_case(n, k, values, exists, [lo] + sample[5:50] + [hi])
    cases["largest present last"] = list_case(n, k, values, exists, sample[3:36] + [hi])
    cases["one above and one below"] = list_case(n, k, values, exists, [v for v in (mid - 1, mid + 1) if v not in everything] + [lo + 1, hi - 1])
    cases["negate"] = list_case(n, k, values, exists, sample[:300], negate=True)
    if k < 64:
        beyond = [(1 << k) + mid, (1 << k) + hi, 1 << k, U64_MAX] + ([(1 << 32) + mid] if k < 32 else [])
        cases["beyond the width"] = list_case(n, k, values, exists, sample[:7] + beyond)
        cases["only beyond the width"] = list_case(n, k, values, exists, beyond)
    else:
        planted, exists = _bsi.plant(values, rng, [U64_MAX, 0, 1 << 63], exists)
        cases["2^64 - 1"] = list_case(n, k, planted, exists, [0, 1 << 63, U64_MAX, U64_MAX])
    return cases


def bitset_edges(k=24, n=SEG_WORDS + 5, with_exists=True):
    """name -> case: set_bits in {0, 1, 31, 32, 33, 2^20 + 5} with the last word's spare bits all ones, values at set_bits - 1 and at
    set_bits planted; a domain narrower than the slices."""
    cases = {}
    for set_bits in (0, 1, 31, 32, 33, (1 << 20) + 5):
        if set_bits > 1 << k:
            continue
        values, exists, rng = attribute(n, k, with_exists, 3, domain=set_bits + 3)
        wanted = [v for v in (set_bits - 1, set_bits, set_bits + 1, 32 * ((set_bits + 31) // 32) - 1) if 0 <= v < 1 << k]
        values, exists = _bsi.plant(values, rng, wanted, exists)
        c = bitset_case(n, k, values, exists, set_bits, rng)
        if set_bits:
            c["words"][(set_bits - 1) >> 5] |= np.uint32(1 << ((set_bits - 1) & 31))  # the last bit of the domain is in the set
        cases[f"set_bits {set_bits}"] = c
        cases[f"set_bits {set_bits} negated"] = dict(c, negate=True)
    return cases


def seam_case(k=40, negate=False):
    """Above 32 slices: matches planted in groups 511 and 512 of a segment and in the last valid group of a ragged last segment,
    values that differ from a set entry in their high half only, and an existence bitmap with a whole empty segment."""
    n = SEG_WORDS * 3 + 40
    values, exists, rng = attribute(n, k, True, 4)
    groups = (32 * n + 30) // 31
    entries = [(0xABCDE << 20) | 0x12345, (1 << (k - 1)) | 77, 5]
    rows = [31 * 511 + 30, 31 * 512, 2 * SEG_BITS + 31 * 511 + 7, 2 * SEG_BITS + 31 * 512 + 3, 31 * (groups - 1), 32 * n - 1]
    for i, r in enumerate(rows):
        values[r] = np.uint64(entries[i % 3])
        exists[r] = True
    values[100] = np.uint64(entries[0] ^ (1 << 32))  # the same low half: no match
    values[31 * 600 + 2] = np.uint64(entries[2] | (1 << 35))
    exists[[100, 31 * 600 + 2]] = True
    exists[SEG_BITS: 2 * SEG_BITS] = False
    return list_case(n, k, values, exists, entries + [int(v) for v in values[1000:1040]], negate)


def named_cases():
    """name -> case: what tests/test_member_reference.py proves the restatement and the wrong models on."""
    cases = {}
    for n in (1, 31, SEG_WORDS, SEG_WORDS * 3 + 5):
        for k in (1, 2, 20, 32, 33, 63, 64):
            for with_exists in (False, True):
                cases[f"headline {n} x {k}{' exists' if with_exists else ''}"] = headline(n, k, with_exists, negate=(n + k) % 2 == 1)
            cases[f"headline bit array {n} x {k}"] = headline(n, k, k % 2 == 0, negate=n == 31, bitset=True)
    for prefix, made in (("list", list_edges()), ("list 64", list_edges(64, 40)), ("list 33", list_edges(33, 40, False)), ("bit array", bitset_edges()),
                         ("bit array 40", bitset_edges(40, 40))):
        cases.update({f"{prefix}: {name}": c for name, c in made.items()})
    cases["seam"] = seam_case()
    cases["seam negated"] = seam_case(negate=True)
    return cases


# the named case on which a wrong model has to change the answer
CAUGHT_BY = {
    "last entry never compared": "list: largest present last",
    "capacity for the count": "list: count 2 poisoned",
    "spare bits honoured": "bit array: set_bits 33",
    "negate without existence": "list: negate",
    "cut to 32 bits": "seam",
    "modulo the width": "list: only beyond the width",
    "second half over the first": "seam",
}

"""Streams that decode to more than 2^32 groups, and a piecewise reference for their multi-GB outputs.

TEST INFRASTRUCTURE (tests/test_wide_reference.py, tests/test_gpu_wide_streams.py).

Decoding is concatenative at 32-group boundaries: 32 groups are exactly 31 output words.  A stream is built here as a list
of PIECES, each of which starts on such a boundary and holds a multiple of 32 groups:
  fill piece  one fill word whose count is a multiple of 32: 31 * count / 32 words of 0x00000000 or 0xFFFFFFFF;
  word piece  a short stream (oracle.compress of a bitmap of 31 k words, k groups of 32): oracle.decompress(piece).
The expected output is then known piece by piece, and a device output is checked against the pieces ON THE DEVICE, in
chunks of at most 2^28 words: nothing of the output goes to the host, nothing is decoded on the CPU but the word pieces.
"""
import bisect

import numpy as np

FILL0 = 0x80000000
FILL1 = 0xC0000000
MAX_COUNT = (1 << 30) - 1
CHUNK_WORDS = 1 << 28  # largest slice of the output one comparison looks at
TILE_WORDS = 4096      # an expand tile of the decoder (kScanTileWords)
PASS_TILE_WORDS = 8192  # a tile of the one-pass decoder (two expand tiles)


class WideStream:
    """A stream built piece by piece, with the output it must decode to."""

    def __init__(self, oracle, name=""):
        self.oracle = oracle
        self.name = name
        self._words = []    # stream words, one array per piece
        self.kinds = []     # "fill" / "words"
        self.starts = []    # output word of every piece's first word
        self.lengths = []   # output words of every piece
        self.values = []    # fill piece: its 32-bit word value; word piece: the decoded words (numpy uint32)
        self.c_words = 0    # stream words so far
        self.groups = 0     # groups so far
        self._plan = None
        self._dev_cache = {}

    # ---- building -------------------------------------------------------------------------------------------------------
    def _add(self, kind, words, groups, value, n_out):
        assert groups % 32 == 0 and groups > 0, (kind, groups)
        self._words.append(np.asarray(words, np.uint32))
        self.kinds.append(kind)
        self.starts.append(self.groups // 32 * 31)
        self.lengths.append(n_out)
        self.values.append(value)
        self.c_words += len(words)
        self.groups += groups
        self._plan = None

    def fill(self, ones, count):
        """One fill word of `count` groups (a multiple of 32)."""
        count = int(count)
        assert count % 32 == 0 and 0 < count <= MAX_COUNT, count
        self._add("fill", [(FILL1 if ones else FILL0) | count], count, 0xFFFFFFFF if ones else 0, count // 32 * 31)

    def fills(self, ones, counts):
        for o, c in zip(ones, counts):
            self.fill(bool(o), c)

    def data(self, bitmap):
        """oracle.compress of a bitmap of 31 k words: 32 k groups, decoding to the bitmap itself."""
        bitmap = np.ascontiguousarray(bitmap, np.uint32)
        assert bitmap.size % 31 == 0 and bitmap.size, bitmap.size
        comp = self.oracle.compress(bitmap)
        groups = self.oracle.decoded_groups(comp)
        assert groups == bitmap.size // 31 * 32
        self._add("words", comp, groups, bitmap.copy(), bitmap.size)

    def pad_to(self, stream_word):
        """Fill words of 32 zero groups up to stream word `stream_word`."""
        assert stream_word >= self.c_words, (stream_word, self.c_words)
        while self.c_words < stream_word:
            self.fill(False, 32)

    # ---- what the stream is and decodes to ---------------------------------------------------------------------------
    def stream(self):
        return np.concatenate(self._words).astype(np.uint32) if self._words else np.zeros(0, np.uint32)

    def expected(self):
        """(decoded words, groups): every piece holds whole 32-group blocks, so the words are exactly 31 * groups / 32."""
        return self.groups // 32 * 31, self.groups

    @property
    def words(self):
        return self.expected()[0]

    def expected_host(self):
        """The whole expected output in host memory: only for streams built at a reduced scale."""
        words = self.words
        assert words <= 1 << 26, "a multi-GB output is checked on the device (check()), never built on the host"
        out = np.empty(words, np.uint32)
        for s, n, v in zip(self.starts, self.lengths, self.values):
            out[s: s + n] = v
        return out

    def piece_at(self, word):
        """Index of the piece that output word `word` belongs to."""
        return bisect.bisect_right(self.starts, word) - 1

    def describe(self, i):
        kind, n = self.kinds[i], self.lengths[i]
        what = f"fill of {'ones' if self.values[i] else 'zeros'}, {n // 31 * 32} groups" if kind == "fill" else "word piece"
        return f"piece {i} ({what}; output words {self.starts[i]} .. {self.starts[i] + n})"

    def _batches(self):
        """Consecutive fill pieces of one length become ONE batch (checked as rows of a reshape), word pieces stay single."""
        if self._plan is None:
            plan = []
            i = 0
            while i < len(self.kinds):
                if self.kinds[i] == "words":
                    plan.append(("words", i, 1))
                    i += 1
                    continue
                j = i
                while j < len(self.kinds) and self.kinds[j] == "fill" and self.lengths[j] == self.lengths[i]:
                    j += 1
                plan.append(("fill", i, j - i))
                i = j
            self._plan = plan
        return self._plan

    def check(self, out, device_tag=""):
        """out: a device tensor of 32-bit words holding at least the decoded words.  Compares every word with the pieces on
        the device, at most CHUNK_WORDS words per comparison; on a mismatch raises AssertionError naming the first wrong word
        and its piece."""
        import torch

        words = self.words
        assert out.numel() >= words, (out.numel(), words)
        dev = out.device

        def fail(at, got):
            i = self.piece_at(at)
            v = self.values[i]
            want = v if self.kinds[i] == "fill" else int(v[at - self.starts[i]])
            raise AssertionError(f"{self.name}{device_tag}: first wrong word {at} is {got & 0xFFFFFFFF:#010x}, expected {want:#010x}, "
                                 f"in {self.describe(i)}")

        for kind, i, m in self._batches():
            s = self.starts[i]
            if kind == "words":
                key = ("words", i, str(dev))
                if key not in self._dev_cache:
                    self._dev_cache[key] = torch.from_numpy(self.values[i].view(np.int32)).to(dev)
                want = self._dev_cache[key]
                for lo in range(0, want.numel(), CHUNK_WORDS):
                    got = out[s + lo: s + lo + min(CHUNK_WORDS, want.numel() - lo)]
                    bad = got != want[lo: lo + got.numel()]
                    if bool(bad.any()):
                        k = int(bad.nonzero()[0, 0])
                        fail(s + lo + k, int(got[k]))
                continue
            L = self.lengths[i]
            key = ("fill", i, str(dev))
            if key not in self._dev_cache:
                vals = np.array(self.values[i: i + m], np.uint32).view(np.int32)
                self._dev_cache[key] = torch.from_numpy(vals).to(dev)
            vals = self._dev_cache[key]
            if L <= CHUNK_WORDS:
                rows = CHUNK_WORDS // L
                for r0 in range(0, m, rows):
                    k = min(rows, m - r0)
                    blk = out[s + r0 * L: s + (r0 + k) * L].view(k, L)
                    bad = blk != vals[r0: r0 + k, None]
                    if bool(bad.any()):
                        f = int(bad.view(-1).nonzero()[0, 0])
                        fail(s + r0 * L + f, int(blk.view(-1)[f]))
            else:  # (one fill longer than a chunk)
                for r in range(m):
                    v = int(vals[r])
                    for lo in range(0, L, CHUNK_WORDS):
                        got = out[s + r * L + lo: s + r * L + min(lo + CHUNK_WORDS, L)]
                        bad = got != v
                        if bool(bad.any()):
                            k = int(bad.nonzero()[0, 0])
                            fail(s + r * L + lo + k, int(got[k]))
        return words


# ---- the streams ------------------------------------------------------------------------------------------------------------
def scaled(count, shift):
    """A group count of the full-size stream at a scale of 2^-shift: a multiple of 32, at least 32."""
    return count if shift == 0 else max(32, (count >> shift) // 32 * 32)


def _kinds(rng, n):
    """Kinds of n fills in runs of one to sixteen of the same kind (so that merging them has something to do)."""
    out = np.empty(n, bool)
    i, k = 0, bool(rng.integers(2))
    while i < n:
        r = int(rng.integers(1, 17))
        out[i: i + r] = k
        i += r
        k = not k
    return out


def _ordinary(ws, oracle, seed):
    """Dense, sparse (p = 2^-10) and clustered data, each a multiple of 31 words long."""
    ws.data(oracle.gen_uniform(31 * 151, seed, 0.5))
    ws.data(oracle.gen_uniform(31 * 2003, seed + 1, 2.0 ** -10))
    ws.data(oracle.gen_clustered(31 * 2011, seed + 2))


def _lead_in(ws, oracle, seed, region_at):
    """Ordinary data, then padding up to stream word `region_at`, with the groups in front of the region NOT a multiple of
    1024 (segments then straddle the region's edges)."""
    _ordinary(ws, oracle, seed)
    ws.pad_to(region_at - 1)
    ws.fill(False, 32 if (ws.groups + 32) % 1024 else 64)
    assert ws.c_words == region_at and ws.groups % 1024 != 0


def giant_case(oracle, case, shift=0, seed=0):
    """The streams of tests/test_gpu_wide_streams.py: ordinary data, a giant region, ordinary data.  Every fill of the region
    holds at most 2^25 groups (the one-pass decoder's bucket sums then hold the tile's counts), except where stated.
      C1  one expand tile of 2^31 - 2^20 groups
      C2  one expand tile of 2^31 + 2^20 groups
      C3  one expand tile of 4096 fills of 2^20 groups: exactly 2^32
      C4  one expand tile of 2^32 + 2^31 - 2^26 groups, among them one bucket (64 words) of 64 fills of exactly 2^25 groups
          (2^31: the largest bucket that is not saturated); the data behind it lies beyond 2^32 output words
      C5  C3 with one fill of 2^25 + 32 groups: that bucket saturates, the tile is staged whole
      C6  the fills of C3 across the end of a one-pass tile: 1000 fills in one expand tile, 3096 in the next
    shift: counts divided by 2^shift (tests/test_wide_reference.py builds the streams small enough to decode on the CPU)."""
    rng = np.random.default_rng(1000 + 17 * seed + ord(case[-1]))
    ws = WideStream(oracle, f"{case}{'' if shift == 0 else f' (1/2^{shift})'}")
    # the region's first stream word: a one-pass tile's first or second half, or (C6) 1000 words in front of a one-pass tile's end
    region_at = {"C1": 2 * PASS_TILE_WORDS, "C2": 2 * PASS_TILE_WORDS + TILE_WORDS, "C3": 2 * PASS_TILE_WORDS,
                 "C4": 2 * PASS_TILE_WORDS + TILE_WORDS, "C5": 2 * PASS_TILE_WORDS, "C6": 3 * PASS_TILE_WORDS - 1000}[case]
    _lead_in(ws, oracle, 10 * seed + 1, region_at)
    u = 1 << 20
    if case == "C1":
        counts = [u // 2] * 4092 + [u // 4] * 4                 # 2^31 - 2^21 + 2^20
    elif case == "C2":
        counts = [u // 2] * 4092 + [u // 2 + u // 4] * 4        # 2^31 - 2^21 + 3 * 2^20
    elif case in ("C3", "C6"):
        counts = [u] * 4096
    elif case == "C4":
        counts = [u] * 4096
        counts[64 * 40: 64 * 41] = [1 << 25] * 64               # bucket 40 of the tile
    elif case == "C5":
        counts = [u] * 4096
        counts[1234] = (1 << 25) + 32
    else:
        raise ValueError(case)
    kinds = _kinds(rng, len(counts))
    ws.region_piece = len(ws.kinds)  # index of the region's first piece
    if case == "C4":
        kinds[64 * 40: 64 * 41] = True  # one run of 2^31 ones: the merged stream cuts it at multiples of 2^29, beyond 2^32
    ws.fills(kinds, [scaled(c, shift) for c in counts])
    ws.region = (region_at, region_at + len(counts))
    _ordinary(ws, oracle, 10 * seed + 5)
    return ws


GIANT_CASES = ("C1", "C2", "C3", "C4", "C5", "C6")

# the sums pass saturates at 2^47 groups (kSumSaturate): 131 072 fills of 2^30 - 32 groups stay below it, one more does not
SUM_LIMIT_FILL = FILL1 | ((1 << 30) - 32)
SUM_LIMIT_FILLS = 1 << 17


def sum_limit_stream(extra=0, shift=0):
    """131 072 (+ extra) fills of 2^30 - 32 groups, alternating kinds: 2^47 - 2^22 groups (+ extra fills' worth)."""
    count = scaled((1 << 30) - 32, shift)
    st = np.empty(SUM_LIMIT_FILLS + extra, np.uint32)
    st[0::2] = FILL1 | count
    st[1::2] = FILL0 | count
    groups = st.size * count
    return st, ((31 * groups + 31) // 32, groups)

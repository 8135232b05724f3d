"""GPU tests: the kernels AT their switch points -- the exact counts, totals and capacities at which they change code -- on
every route and pointer alignment.

tests/_switch.py builds the inputs and lists the switches (its docstring holds the table); tests/test_switch_reference.py
proves on the CPU that the inputs have the counts they claim and that the probes sit on both sides of every switch.  Here
every probe is compared word for word with the CPU oracle (oracle.compress / oracle.decompress, _py_merge_fills for the
unsegmented form); the one exception is stated at test_bitops_with_more_than_1024_tiles.

Which test sits on which switch:
  pair count 384, 2048 + all literals, 256 t < count                         test_pair_counts_*
  pair slot of a wave; kernel instances <1,1> <2,2> <3,3> <3,1> <3,2>,       test_pair_counts_compress (SHAPE_CASES: the probes in every size
    kAligned true and false; two pairs per wave on the no-wait routes          class of compress_tile_shape; input offsets 0, 4, 8, 12 bytes)
  one / two / five segments per wave of compress_tile_body                   test_pair_counts_bitop_tile_kernels, ..._kernel_shapes
  descriptor cut at min(room, count); capacity == C, C - 1                   test_exact_capacity_*
  4-byte aligned inputs and outputs                                          test_pointer_offsets_*
  one-pass tile of 61439 / 61440 / 61441 groups, a single clamped count      test_one_pass_tile_limit, test_tiles_around_the_limit_in_turn
  out_capacity 7 c, 7 c + 1, 40 c, 40 c + 1                                  test_default_decoder_route
  112 words per segment (run merge or decode-based bit operation)            test_bitop_route_limit
  256 / 128 / 64 segments per workgroup                                      test_bitop_runs_tile_shapes
  a tile of exactly the LDS image's words, one more, far more               test_bitop_runs_tile_of_exactly_the_lds_image, test_bitop_runs_tile_beyond_the_lds_image
  more than 1024 tiles: the scans' second round                              test_bitops_with_more_than_1024_tiles, test_no_wait_decoder_beyond_one_scan_round
  the operand-list bit operation (wah_bitop_list.hip; expected: the numpy fold of the operand bitmaps through oracle.compress,
  the index as _Case computes it, an output of exactly C words between sentinels):
    128 words a batch, the fast path of a full batch of literals             test_list_segment_words, test_list_stream_offsets
    fills of 1 .. 8 groups by their lane, 9 and more by the wave, 64 a step  test_list_fill_groups
    kListDepth = 4 batches in flight, settled operands                       test_list_batch_schedules
    64 operands a chunk, m_first for row 0 alone                             test_list_operand_counts, test_list_operand_positions
    the settled one-word segment, nvalid < 1024                              test_list_ragged_ends, test_list_refused_identity_fill_of_another_length
    kSegDecodeWaves = 4 segments a workgroup                                 test_list_segment_counts
    1023 / 1025 groups, the count clamp, empty fills, bad rows 63 / 64 / 4096 test_list_refusals_at_the_boundaries, test_list_refused_rows
"""
import functools

import numpy as np
import pytest

from tests import _oracle, _switch as sw
from tests.test_gpu_parity import (_dev, _host, _indexed_stream, _py_merge_fills, _random_foreign_stream, _route_is,  # noqa: F401
                                   _run_structured_bitmap, _whole_stream_equals_oracle, wah)  # (wah: the fixture)
from tests.test_gpu_wide_streams import ROUTES, _Decoder

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 64  # sentinel words in front of and behind an output
WAH_ERR_CAPACITY = -4

# compressor route -> (entry point, flags, the stream is the unsegmented form)
COMPRESS_ROUTES = {"plain": ("device", 0, False), "indexed": ("indexed", 0, False), "no wait": ("ex", 2, False),
                   "unsegmented": ("ex", 1, True), "unsegmented no wait": ("ex", 3, True)}
FOLD = {"and": lambda xs: np.bitwise_and.reduce(xs), "or": lambda xs: np.bitwise_or.reduce(xs),
        "xor": lambda xs: np.bitwise_xor.reduce(xs), "andnot": lambda xs: xs[0] & ~np.bitwise_or.reduce(xs[1:]) if len(xs) > 1 else xs[0]}


# ---- helpers ----------------------------------------------------------------------------------------------------------------
class _Case:
    """A bitmap with what the oracle makes of it: the stream, its unsegmented form, the segment index, the decoded words."""

    def __init__(self, name, bitmap):
        oracle = _oracle.load()
        self.name = name
        self.bitmap = np.ascontiguousarray(bitmap, np.uint32)
        self.n = int(self.bitmap.size)
        self.want = oracle.compress(self.bitmap)
        whole = self.n // sw.SEG_WORDS  # (an all-zero segment is one fill word: no call for the padding of the large cases)
        zero = ~self.bitmap[: whole * sw.SEG_WORDS].reshape(whole, sw.SEG_WORDS).any(axis=1)
        lengths = [1 if lo < whole * sw.SEG_WORDS and zero[lo // sw.SEG_WORDS] else oracle.compress(self.bitmap[lo: lo + sw.SEG_WORDS]).size
                   for lo in range(0, self.n, sw.SEG_WORDS)]
        self.index = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        assert self.index[-1] == self.want.size

    @functools.cached_property
    def decoded(self):
        return _oracle.load().decompress(self.want)

    @functools.cached_property
    def merged(self):
        return _py_merge_fills(self.want)

    def expected(self, route):
        return self.merged if COMPRESS_ROUTES[route][2] else self.want


def _at_offset(words, offset, room=0):
    """A device copy of `words` (+ room words behind) that starts `offset` words behind a 16-byte boundary; returns the view."""
    import torch

    buf = torch.zeros(offset + len(words) + room + 4, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset: offset + len(words) + room]
    view[: len(words)] = _dev(words)
    assert view.data_ptr() % 16 == 4 * offset
    return view


class _Compressor:
    """Workspace, count and index output for bitmaps of up to n words; run() goes through the C ABI with the caller's pointers."""

    def __init__(self, wah, n):
        import torch

        self.lib = wah.lib()
        self.ws_bytes = int(self.lib.wah_compress_workspace_bytes(n))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.offsets = torch.zeros((wah.max_compressed_words(n) + 1023) // 1024 + 1, dtype=torch.int64, device="cuda")

    def run(self, route, d_in, n, out, capacity):
        """Returns (status, C as the launch reports it)."""
        entry, flags, _ = COMPRESS_ROUTES[route]
        lib, ws = self.lib, self.ws.data_ptr()
        self.count.fill_(-1)
        if entry == "device":
            rc = lib.wah_compress_device(d_in.data_ptr(), n, out.data_ptr(), capacity, self.count.data_ptr(), ws, self.ws_bytes, None)
        elif entry == "indexed":
            self.offsets.fill_(-1)
            rc = lib.wah_compress_device_indexed(d_in.data_ptr(), n, out.data_ptr(), capacity, self.count.data_ptr(),
                                                 self.offsets.data_ptr(), ws, self.ws_bytes, None)
        else:
            rc = lib.wah_compress_device_ex(d_in.data_ptr(), n, out.data_ptr(), capacity, self.count.data_ptr(), flags, ws,
                                            self.ws_bytes, None)
        assert rc == 0, (route, rc, lib.wah_last_error().decode())
        return int(lib.wah_compress_status(ws, None)), int(self.count.item())


def _guarded(words, offset=0):
    """(whole buffer, the view of `words` words at GUARD + offset words behind a 16-byte boundary), all sentinel."""
    import torch

    buf = torch.full((GUARD + offset + words + GUARD + 4,), SENTINEL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0 and GUARD % 4 == 0
    return buf, buf[GUARD + offset: GUARD + offset + words]


def _untouched(buf, view, written):
    """Everything of buf outside view[:written] still holds the sentinel."""
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + written:] == SENTINEL).all())


def _check_compress(case, comp, route, d_in, out_offset=0, tag=""):
    """One compress launch of `case` by `route` into an output of exactly C words: status, C, every word, the index, the guards."""
    want = case.expected(route)
    buf, out = _guarded(want.size, out_offset)
    status, c = comp.run(route, d_in, case.n, out, want.size)
    what = f"{case.name} [{route}{tag}]"
    assert status == 0 and c == want.size, (what, status, c, want.size)
    got = _host(out)
    if not np.array_equal(got, want):
        bad = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: compressed word {bad} is {got[bad]:#010x}, the oracle's {want[bad]:#010x}")
    assert _untouched(buf, out, want.size), f"{what}: written outside the output"
    if route == "indexed":
        offs = comp.offsets.cpu().numpy()[: case.index.size]
        assert np.array_equal(offs, case.index), (what, int(np.flatnonzero(offs != case.index)[0]))


def _decode_routes(wah, name, stream, want, groups, stream_offset=0, out_offset=0, capacity=None, routes=ROUTES):
    """`stream` through every decoder route into an output of `capacity` (default: exactly the decoded) words: status, route,
    info, every word, the guards.  stream_offset: the stream starts that many words behind a 16-byte boundary (the route is
    then the two launches unless it is the no-wait one)."""
    capacity = want.size if capacity is None else capacity
    dec = _Decoder(wah, stream, capacity, offset=stream_offset)
    for route in routes:
        if stream_offset and route == "4-byte aligned":
            continue  # (that route is dec.d_odd: offset 1, part of stream_offset == 0's round)
        buf, out = _guarded(capacity, out_offset)
        status, seen, info = dec.run(route, out)
        what = f"{name} [{route}, stream + {stream_offset}, output + {out_offset}, capacity {capacity}]"
        expect_route = ROUTES[route] if not stream_offset else (3 if route == "no wait" else 2)
        if route == "default" and not stream_offset:  # (by what the capacity allows the stream to be)
            expect_route = sw.default_route(stream.size, capacity)
        assert _route_is(seen, expect_route), (what, seen)
        if capacity < want.size:
            assert status == WAH_ERR_CAPACITY, (what, status)
            assert _untouched(buf, out, capacity), f"{what}: written outside the capacity"
            continue
        assert status == 0, (what, status, dec.error())
        assert info == [want.size, groups], (what, info)
        got = _host(out)
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            raise AssertionError(f"{what}: decoded word {bad} is {got[bad]:#010x}, the oracle's {want[bad]:#010x}")
        assert _untouched(buf, out, want.size), f"{what}: written outside the output"


def _groups(stream):
    return _oracle.load().decoded_groups(stream)


# ---- (a) pair word counts ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_case(which):
    rng = np.random.default_rng(100 + len(which) + sum(map(ord, which)))
    if which.startswith("padding "):
        pad = int(which.split()[1])
        return _Case(f"probe pairs behind {pad} pairs", sw.probe_bitmap(rng, pad)[0])
    if which in sw.SHAPE_CASES:
        return _Case(which, sw.shaped_probe_bitmap(rng, sw.SHAPE_CASES[which][0])[0])
    if which == "lone segment":
        return _Case("ends in a lone segment", sw.ragged_end_bitmap(rng, 0, lone_segment=True))
    words = int(which.split()[1])
    return _Case(f"ends {words} words into a pair's second segment", sw.ragged_end_bitmap(rng, words))


PAIR_CASES = [f"padding {p}" for p in sw.PAIR_PADDINGS] + [f"tail {w}" for w in sw.LAST_SEGMENT_WORDS] + ["lone segment"]


@pytest.mark.parametrize("which", PAIR_CASES + list(sw.SHAPE_CASES))
def test_pair_counts_compress(wah, which):
    """Every pair count of tests/_switch.py PAIR_COUNTS x split x placement, the full pairs with one fill group, and bitmaps
    that end inside a pair: through the plain, indexed (EVERY index entry), no-wait, unsegmented and unsegmented no-wait
    compressors with the input 0, 4, 8 and 12 bytes behind a 16-byte boundary (the kAligned = false instance of each kernel),
    and the host compress().  The pair slot depends on the bitmap's size (compress_tile_shape): the "padding" bitmaps are one
    pair per wave on the one-launch routes (two, both slots, on the no-wait routes); the SHAPE_CASES put the same probes
    behind all-zero pairs into the classes of two and of three pairs per wave and into the tails of one and of two behind a
    full round of three, shifted so that every probe meets every slot: the instances <1,1>, <2,2>, <3,3>, <3,1>, <3,2> of
    compress_pair_kernel and compress_unseg_pair_kernel, kAligned true and false."""
    import torch

    case = _pair_case(which)
    if which in sw.SHAPE_CASES:  # the shape this device gives the bitmap is the one the case is named for
        slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
        assert sw.tile_shape((case.n + 2 * sw.SEG_WORDS - 1) // (2 * sw.SEG_WORDS), slots)[:2] == sw.SHAPE_CASES[which][1], (which, slots)
    comp = _Compressor(wah, case.n)
    for offset in range(4):
        d_in = _at_offset(case.bitmap, offset)
        for route in COMPRESS_ROUTES:
            _check_compress(case, comp, route, d_in, tag=f", input + {4 * offset} bytes")
    got = wah.compress(case.bitmap)
    assert got.shape == case.want.shape and np.array_equal(got, case.want), case.name


@pytest.mark.parametrize("which", PAIR_CASES)
def test_pair_counts_bitop_tile_kernels(wah, oracle, which):
    """The same group patterns through compress_tile_body (wah_bitop_device's and the indexed decode-based route's compress
    stage): A or 0 == A, the stream and the index."""
    case = _pair_case(which)
    zeros = oracle.compress(np.zeros(case.n, np.uint32))
    z_index = np.arange(case.index.size, dtype=np.int64)  # one fill word per segment
    assert zeros.size == z_index.size - 1
    got = _host(wah.bitop_device("or", _dev(case.want), _dev(zeros), case.n))
    assert got.shape == case.want.shape and np.array_equal(got, case.want), case.name
    import torch

    assert case.want.size + zeros.size > sw.RUNS_MAX_WORDS_PER_SEG * (case.index.size - 1)
    got, offs = wah.bitop_indexed_device("or", _dev(case.want), torch.from_numpy(case.index).cuda(), _dev(zeros),
                                         torch.from_numpy(z_index).cuda(), case.n)
    assert wah.lib().wah_last_bitop_route() == 2
    assert got.numel() == case.want.size and np.array_equal(_host(got), case.want), case.name
    assert np.array_equal(offs.cpu().numpy()[: case.index.size], case.index), case.name


@pytest.mark.parametrize("which", ["two pairs per wave, shift 0", "three pairs per wave, shift 0", "three pairs per wave, shift 1"])
def test_pair_counts_bitop_tile_kernel_shapes(wah, oracle, which):
    """compress_tile_body takes one, two or five segments per wave by the bitmap's size (compress_wave_segs; the PAIR_CASES
    above are all one): the probe pairs through wah_bitop_device in the classes of two and of five."""
    case = _pair_case(which)
    assert sw.wave_segs(case.index.size - 1) == (2 if which.startswith("two") else 5)
    zeros = oracle.compress(np.zeros(case.n, np.uint32))
    for op, other in (("or", zeros), ("and", oracle.compress(np.full(case.n, 0xFFFFFFFF, np.uint32)))):
        got = _host(wah.bitop_device(op, _dev(case.want), _dev(other), case.n))
        assert got.shape == case.want.shape and np.array_equal(got, case.want), (case.name, op)


@pytest.mark.parametrize("which", PAIR_CASES)
def test_pair_counts_decode(wah, which):
    """The oracle's stream of every probe bitmap on every decoder route, and through the segment index."""
    import torch

    case = _pair_case(which)
    _decode_routes(wah, case.name, case.want, case.decoded, _groups(case.want))
    back = wah.decompress_segments_device(_dev(case.want), torch.from_numpy(case.index).cuda(), case.n)
    assert np.array_equal(_host(back)[: case.n], case.bitmap), case.name
    _decode_routes(wah, case.name + " (unsegmented)", case.merged, case.decoded, _groups(case.want), routes=("default", "two launches", "no wait"))


# ---- (b) exact capacity -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _capacity_cases():
    oracle = _oracle.load()
    rng = np.random.default_rng(7)
    base = np.concatenate([oracle.gen_uniform(992 * 37, 3, 0.03), sw.pair(2048, "even", "front", 0, rng), oracle.gen_uniform(992 * 50, 4, 0.5)])
    cases = [_Case(f"C mod 4 case {w}", np.concatenate([base, sw.segment(w, "spread", 1, rng), rng.integers(0, 2**32, 77, dtype=np.uint64).astype(np.uint32)]))
             for w in (1, 2, 3, 4)]
    assert sorted(c.want.size % 4 for c in cases) == [0, 1, 2, 3]
    return cases


@pytest.mark.parametrize("route", list(COMPRESS_ROUTES))
def test_exact_capacity_compress(wah, route):
    """out_capacity == C (for C mod 4 = 0 .. 3): WAH_OK, the oracle's stream, nothing outside it; out_capacity == C - 1:
    WAH_ERR_CAPACITY and nothing behind the capacity."""
    for case in _capacity_cases():
        comp = _Compressor(wah, case.n)
        d_in = _dev(case.bitmap)
        _check_compress(case, comp, route, d_in)
        want = case.expected(route)
        buf, out = _guarded(want.size)
        status, c = comp.run(route, d_in, case.n, out, want.size - 1)
        assert status == WAH_ERR_CAPACITY and c == want.size, (case.name, route, status, c)
        assert _untouched(buf, out, want.size - 1), f"{case.name} [{route}]: written behind a capacity of C - 1"


def test_exact_capacity_decode(wah):
    """capacity == the decoded words: WAH_OK, every word, nothing behind; one word less: WAH_ERR_CAPACITY, nothing behind."""
    for case in _capacity_cases():
        for capacity in (case.decoded.size, case.decoded.size - 1):
            _decode_routes(wah, case.name, case.want, case.decoded, _groups(case.want), capacity=capacity)


# ---- (c) pointer offsets ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _offset_cases():
    oracle = _oracle.load()
    n = 992 * 2 * 24 * 3 + 992 * 5 + 13  # a few tiles and a ragged end
    return [_Case("sparse", oracle.gen_uniform(n, 5, 2.0 ** -9)), _Case("incompressible", oracle.gen_uniform(n, 6, 0.5))]


@pytest.mark.parametrize("route", list(COMPRESS_ROUTES))
def test_pointer_offsets_compress(wah, route):
    """Input and output each 0 .. 3 words behind a 16-byte boundary (include/wah.h: 4-byte alignment is all the device calls
    need; the stores go through descriptors with a dword-aligned base): the oracle's stream, sentinels in front and behind."""
    for case in _offset_cases():
        comp = _Compressor(wah, case.n)
        for in_off in range(4):
            d_in = _at_offset(case.bitmap, in_off)
            for out_off in range(4):
                _check_compress(case, comp, route, d_in, out_off, tag=f", input + {in_off} words, output + {out_off} words")


@pytest.mark.parametrize("stream_offset", range(4))
def test_pointer_offsets_decode(wah, stream_offset):
    """The stream and the output each 0 .. 3 words behind a 16-byte boundary, on every decoder route; a stream that is not
    16-byte aligned goes by the two launches."""
    for case in _offset_cases():
        for out_off in range(4):
            _decode_routes(wah, case.name, case.want, case.decoded, _groups(case.want), stream_offset, out_off)


def test_pointer_offsets_index_decode(wah):
    """wah_decompress_segments_device with the stream and the output each 0 .. 3 words behind a 16-byte boundary: every
    word, sentinels in front of and behind the output."""
    import torch

    for case in _offset_cases():
        index = torch.from_numpy(case.index).cuda()
        for stream_off in range(4):
            d = _at_offset(case.want, stream_off)
            for out_off in range(4):
                buf, out = _guarded(case.decoded.size, out_off)
                got = wah.decompress_segments_device(d, index, case.n, out=out)
                assert np.array_equal(_host(got), case.decoded) and _untouched(buf, out, case.decoded.size), (case.name, stream_off, out_off)


# ---- (d) the one-pass decoder's tile limit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("way", sw.TILE_WAYS)
@pytest.mark.parametrize("total", sw.TILE_TOTALS)
def test_one_pass_tile_limit(wah, oracle, total, way):
    """A tile of exactly 61439 / 61440 / 61441 groups (one word of that count: the clamp), as the first, a middle, a batch's
    second and the last tile, between plain literal tiles, on every route."""
    rng = np.random.default_rng(total)
    for place in sw.TILE_PLACES:
        st, t, groups = sw.tile_limit_stream(total, way, place, rng)
        _decode_routes(wah, f"tile {t} ({place}) of {groups} groups by {way}", st, oracle.decompress(st), oracle.decoded_groups(st))


def test_tiles_around_the_limit_in_turn(wah, oracle):
    """Tiles of 61440 and 61441 groups in turn (own expansion and deferred list interleave at every tile), and a tile far
    under the limit that is deferred for its one empty fill."""
    rng = np.random.default_rng(11)
    for name, st in (("61440 / 61441 in turn", sw.alternating_tile_stream(rng)), ("an empty fill", sw.tile_with_empty_fill(rng))):
        _decode_routes(wah, name, st, oracle.decompress(st), oracle.decoded_groups(st))


# ---- (e) the default decoder route ------------------------------------------------------------------------------------------
def test_default_decoder_route(wah, oracle):
    data = oracle.gen_uniform(992 * 20 + 5, 9, 0.5)
    st = oracle.compress(data)
    want = oracle.decompress(st)
    d = _dev(st)
    for capacity, route in sw.route_capacities(st.size).items():
        dec = wah.DeviceDecompressor(st.size, capacity)
        dec.run(d)
        got = _host(dec.result())
        assert _route_is(dec.route, wah.DeviceDecompressor.ROUTES[route]), (capacity, dec.route)
        assert np.array_equal(got, want), capacity


# ---- (f) bit operations at their limits -------------------------------------------------------------------------------------
def _check_bitop(wah, oracle, maps, n, ops=FOLD, route=None, what=""):
    """Every operation on the operands: the oracle's stream of the combined bitmap, its index, the route."""
    cases = [_Case("operand", m) for m in maps]
    import torch

    operands = [(_dev(c.want), torch.from_numpy(c.index).cuda()) for c in cases]
    for name in ops:
        combined = _Case("combined", FOLD[name](np.stack(maps)).astype(np.uint32))
        got, offs = wah.bitop_many_indexed_device(name, operands, n)
        if route is not None:
            assert wah.lib().wah_last_bitop_route() == route, (what, name, route)
        assert got.numel() == combined.want.size and np.array_equal(_host(got), combined.want), (what, name)
        assert np.array_equal(offs.cpu().numpy()[: combined.index.size], combined.index), (what, name)
    return sum(c.want.size for c in cases)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_bitop_route_limit(wah, oracle, k):
    """Operands whose words total 112 S - 1, 112 S (run merge) and 112 S + 1 (decode-based): the same stream and index."""
    rng = np.random.default_rng(20 + k)
    for s in (64, 70):
        for total, route in sw.runs_totals(s).items():
            maps = sw.operands_with_total(k, s, total, rng)
            assert _check_bitop(wah, oracle, maps, s * sw.SEG_WORDS, route=route, what=(k, s, total)) == total


@pytest.mark.parametrize("s", sw.RUNS_SHAPE_SEGMENTS)
def test_bitop_runs_tile_shapes(wah, oracle, s):
    """Totals just below, at and above the choice of 256, 128 or 64 segments per workgroup, for segment counts that end ON a
    tile, one behind, 63, 64 and 255 behind."""
    rng = np.random.default_rng(s)
    for i, total in enumerate(sw.runs_shape_totals(s)):
        maps = sw.operands_with_total(2 + i % 2, s, total, rng)
        assert _check_bitop(wah, oracle, maps, s * sw.SEG_WORDS, route=1, what=(s, total)) == total


@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_bitop_runs_tile_beyond_the_lds_image(wah, oracle, k):
    """Eight incompressible segments inside sparse operands: that tile's words do not fit the LDS image and are read from
    global memory -- as the first tile and as the last."""
    rng = np.random.default_rng(40 + k)
    for tile in (0, 3):
        maps = sw.operands_with_dense_tile(k, 1024, tile, rng)
        total = _check_bitop(wah, oracle, maps, 1024 * sw.SEG_WORDS, route=1, what=(k, tile))
        image = sw.runs_lds_image_words(total, 1024, 256)  # (the sparse tiles: 2 k words per segment; the dense one: + 8 x 1022)
        assert sw.runs_shape(total, 1024) == 256 and 2 * k * 256 <= image < 2 * k * 256 + 8 * (sw.SEG_GROUPS - 2), (total, image)


@pytest.mark.parametrize("k", [2, 3])
def test_bitop_runs_tile_of_exactly_the_lds_image(wah, oracle, k):
    """A tile whose words equal the LDS image (staged) and one of a word more (read from global memory), first and last tile."""
    rng = np.random.default_rng(50 + k)
    w = sw.lds_boundary_tile_words(k, 1024)
    for tile in (0, 3):
        for words in (w, w + 1):
            maps = sw.operands_with_tile_words(k, 1024, tile, words, rng)
            total = _check_bitop(wah, oracle, maps, 1024 * sw.SEG_WORDS, route=1, what=(k, tile, words))
            assert sw.runs_shape(total, 1024) == 256 and sw.runs_lds_image_words(total, 1024, 256) == w, (k, total)


@pytest.mark.parametrize("shape", [64, 256])
def test_bitops_with_more_than_1024_tiles(wah, oracle, shape):
    """1025 tiles: every thread of bitop_runs_scan_kernel takes two tiles.  64 segments per workgroup: 65 537 segments of 80
    words per segment; 256: 262 145 segments (about 1 GiB) of clustered bits, generated on the device.  The expected stream
    is the oracle's of the combined bitmap, every word (_whole_stream_equals_oracle); the expected INDEX is the indexed
    compressor's of the combined bitmap, whose stream that same comparison ties to the oracle word for word."""
    import torch

    lib = wah.lib()
    if shape == 64:
        s = sw.MANY_TILES_64
        maps = sw.operands_with_total(2, s, 80 * s, np.random.default_rng(64))
        d_maps = [_dev(m) for m in maps]
        del maps
    else:
        s = sw.MANY_TILES_256
        d_maps = [wah.gen_clustered_device(s * sw.SEG_WORDS, 70 + j, 1_500_000 * (j + 1)).clone() for j in range(2)]
    n = s * sw.SEG_WORDS
    operands = [_indexed_stream(wah, d) for d in d_maps]
    total = sum(int(st.numel()) for st, _ in operands)
    assert sw.runs_shape(total, s) == shape and (s + shape - 1) // shape == sw.SCAN_ROUND_TILES + 1, (total, s)
    for name, fn in (("xor", torch.bitwise_xor), ("and", torch.bitwise_and)):
        combined = fn(d_maps[0], d_maps[1])
        got, offs = wah.bitop_many_indexed_device(name, operands, n)
        assert lib.wah_last_bitop_route() == 1
        assert _whole_stream_equals_oracle(oracle, combined, got) == got.numel()
        ref, ref_offs = _indexed_stream(wah, combined)
        assert torch.equal(ref, got) and torch.equal(offs[: ref_offs.numel()], ref_offs), name
        del combined, got, offs, ref, ref_offs
    del operands, d_maps
    torch.cuda.empty_cache()


# ---- (g) the no-wait decoder beyond one round of its table scan ---------------------------------------------------------------
def test_no_wait_decoder_beyond_one_scan_round(wah, oracle):
    """A stream of more than 1024 x 4096 words (the table of the no-wait sums pass is scanned in more than one round): by the
    no-wait route and by the two launches, against the bitmap; and one with a long fill in the second thousand of tiles."""
    import torch

    n = sw.SCAN_ROUND_TILES * 4096 + 4096 * 40 + 17
    d_in = wah.gen_uniform_device(n, 77, 0.5).clone()
    st = wah.compress_device(d_in)
    assert st.numel() > sw.SCAN_ROUND_TILES * 4096
    assert _whole_stream_equals_oracle(oracle, d_in, st) == st.numel()
    foreign = sw.literals(np.random.default_rng(12), sw.SCAN_ROUND_TILES * 4096 + 4096 * 30 + 5)
    foreign[1040 * 4096 + 7] = sw.FILL1 | 5_000_003  # (tiles 1024 .. : the second round of the scan)
    foreign[1031 * 4096] = sw.FILL0 | 70_001
    want = oracle.decompress(foreign)
    for kw, route in (({"no_wait": True}, "no wait"), ({"two_launches": True}, "two launches")):
        dec = wah.DeviceDecompressor(st.numel(), n + 1, **kw)
        dec.run(st)
        back = dec.result()
        assert _route_is(dec.route, route) and back.numel() == (n if n % 31 == 0 else n + 1)
        assert bool(torch.equal(back[:n], d_in)), route
        dec = wah.DeviceDecompressor(foreign.size, want.size, **kw)
        dec.run(_dev(foreign))
        assert np.array_equal(_host(dec.result()), want), route
        assert dec.info.tolist() == [want.size, oracle.decoded_groups(foreign)]


# ---- the suite's fuzz inputs on the routes they did not reach ------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_fuzz_on_every_route(wah, oracle, seed):
    """Random run structures (run lengths around the group, lane, segment and pair sizes) through every compressor route with
    the input on and off a 16-byte boundary, and random foreign streams through every decoder route."""
    rng = np.random.default_rng(6000 + seed)
    n = int(rng.choice([992 * 3 + 1, 992 * 97 + 500, 992 * 2 * 24 * 2 + 31]))
    case = _Case(f"run structures, seed {seed}", _run_structured_bitmap(rng, n, int(rng.choice([3, 20, 200]))))
    comp = _Compressor(wah, case.n)
    for offset in (0, 1 + seed % 3):
        d_in = _at_offset(case.bitmap, offset)
        for route in COMPRESS_ROUTES:
            _check_compress(case, comp, route, d_in, tag=f", input + {offset} words")
    st = _random_foreign_stream(rng, int(rng.choice([3000, 4096 * 2 + 3, 4096 * 9 + 100])), max_groups=8_000_000)
    _decode_routes(wah, f"foreign stream, seed {seed}", st, oracle.decompress(st), oracle.decoded_groups(st))


# ---- (h) the operand-list bit operation at its switch points ----------------------------------------------------------------
WAH_ERR_STREAM = -6


class _ListOperands:
    """Bitmaps as operands of wah_bitop_list_indexed_device: the ORACLE's stream of each and the index computed on the CPU
    (_Case), on the device; a scratch that every call of the object shares."""

    def __init__(self, wah, maps, n):
        import torch

        self.wah, self.n, self.maps = wah, int(n), [np.ascontiguousarray(m, np.uint32) for m in maps]
        assert all(m.size == self.n for m in self.maps)
        self.cases = [_Case("operand", m) for m in self.maps]
        self.dev = [(_dev(c.want), torch.from_numpy(c.index).cuda()) for c in self.cases]
        self.scratch = torch.empty(int(wah.lib().wah_bitop_list_scratch_bytes(self.n, 1)), dtype=torch.uint8, device="cuda")

    def enqueue(self, op, operands, capacity, out_offset=0):
        """One call over `operands` ((stream, index) pairs or a table) into a guarded output of `capacity` words; returns
        (status, C as the launch reports it, buffer, output view, index)."""
        import torch

        wah = self.wah
        table = operands if isinstance(operands, torch.Tensor) else wah.bitop_operand_table(operands)
        buf, out = _guarded(capacity, out_offset)
        n_seg = (self.n + sw.SEG_WORDS - 1) // sw.SEG_WORDS
        offs = torch.full((n_seg + 1,), -1, dtype=torch.int64, device="cuda")
        _, count, _ = wah.bitop_list_indexed_device(op, table, self.n, scratch=self.scratch, out=out, out_offsets=offs, check=False)
        status = int(wah.lib().wah_bitop_list_status(self.scratch.data_ptr(), self.n, int(table.shape[0]), None))
        return status, int(count.item()), buf, out, offs

    def check(self, op, rows, combined, what, operands=None, many=True):
        """The table of rows (indices into the operands) under op: exactly the oracle's stream of `combined` and its index, into
        an output of exactly C words between sentinels; for up to 8 rows also wah_bitop_many_indexed_device's very output."""
        want = _Case("combined", combined)
        assert want.n == self.n
        operands = [self.dev[i] for i in rows] if operands is None else operands
        status, c, buf, out, offs = self.enqueue(op, operands, want.want.size)
        what = f"{what} [{op}, {len(operands)} operands]"
        assert status == 0 and c == want.want.size, (what, status, c, want.want.size)
        got = _host(out)
        if not np.array_equal(got, want.want):
            bad = int(np.flatnonzero(got != want.want)[0])
            seg = int(np.searchsorted(want.index, bad, side="right")) - 1
            raise AssertionError(f"{what}: word {bad} (segment {seg}, its word {bad - int(want.index[seg])}) is {got[bad]:#010x}, the oracle's {want.want[bad]:#010x}")
        assert _untouched(buf, out, want.want.size), f"{what}: written outside the output"
        assert np.array_equal(offs.cpu().numpy(), want.index), (what, "index")
        if many and len(operands) <= 8:
            ref, ref_offs = self.wah.bitop_many_indexed_device(op, operands, self.n)
            assert ref.numel() == c and np.array_equal(_host(ref), got) and np.array_equal(ref_offs.cpu().numpy()[: want.index.size], want.index), (what, "many")

    def fold(self, op, rows, what, **kw):
        self.check(op, rows, FOLD[op](np.stack([self.maps[i] for i in rows])).astype(np.uint32), what, **kw)


def _dense(rng, n_segments):
    """Literals only: every group of the other operand meets a random one, so a group applied wrongly shows."""
    return sw.pack(sw.literals(rng, n_segments * sw.SEG_GROUPS))


@pytest.mark.parametrize("op", sw.LIST_OPS)
def test_list_segment_words(wah, op):
    """Operand segments of every LIST_SEGMENT_WORDS (1, 2, 128 b - 1, 128 b, 128 b + 1, 1023, 1024 words) built every LIST_WAYS
    way -- a fill that ends a full batch, that starts the next one, a fast batch that ends at group 1024 -- alone, as the first
    operand and as a later one of a dense operand, and against the same segments in reverse order."""
    rng = np.random.default_rng(300)
    layouts = [p[3] for p in sw.list_words_probes()]
    probe = sw.list_probe_bitmap(layouts, rng)
    ops = _ListOperands(wah, [probe, _dense(rng, len(layouts)), sw.list_probe_bitmap(layouts[::-1], rng)], probe.size)
    for rows in ([0], [0, 1], [1, 0], [0, 2], [2, 1, 0]):
        ops.fold(op, rows, f"segment words, rows {rows}")


@pytest.mark.parametrize("op", sw.LIST_OPS)
def test_list_fill_groups(wah, op):
    """A fill of every LIST_FILL_GROUPS (1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 700 groups) in every LIST_FILL_WORD_INDEX
    (lane 0's and lane 63's first and second word, of the first and of later batches), of ones and of zeros, and the segments of
    one fill; and batches of many fills (list_many_fills_layouts): alone, in front of and behind a dense operand, and against the
    same segments in reverse order."""
    rng = np.random.default_rng(301)
    layouts = [sw.list_fill_layout(wi, bit, n, total) for wi, bit, n, total in sw.list_fill_probes()] + sw.list_many_fills_layouts()
    probe = sw.list_probe_bitmap(layouts, rng)
    ops = _ListOperands(wah, [probe, _dense(rng, len(layouts)), _dense(rng, len(layouts)), sw.list_probe_bitmap(layouts[::-1], rng)], probe.size)
    for rows in ([0], [0, 1], [1, 0], [1, 0, 2], [0, 3], [3, 1, 0]):
        ops.fold(op, rows, f"fill groups, rows {rows}")


@pytest.mark.parametrize("schedule", sw.LIST_SCHEDULES, ids=lambda s: "-".join(map(str, s)) if len(s) < 12 else f"{len(s)}_operands_{s[-1]}")
def test_list_batch_schedules(wah, schedule):
    """The chunks of LIST_SCHEDULES: 0, 1, 3, 4, 5, 8 and more batches in a chunk of kListDepth = 4 in flight, the producer one
    and two operands ahead of the consumer, settled operands between live ones (the one-word segments are the operation's
    identity under one of the two fill kinds), a chunk of settled operands in front of a live one."""
    rng = np.random.default_rng(302 + len(schedule))
    n_segments = 5 if len(schedule) <= sw.LIST_CHUNK else 2
    for bit in (0, 1):
        maps = sw.list_schedule_operands(schedule, bit, n_segments, rng)
        ops = _ListOperands(wah, maps, n_segments * sw.SEG_WORDS)
        for op in sw.LIST_OPS:
            ops.fold(op, list(range(len(maps))), f"schedule {schedule[:12]}, one-word fills of {bit}")


def _pool_operands(wah, seed):
    """Entries 1 .. of list_pool, and as entries 0 and len(pool) the all-zero and the all-one bitmap."""
    pool = sw.list_pool(np.random.default_rng(seed))
    n = pool[1].size
    pool[0] = sw.list_trivial("or", n)
    pool.append(sw.list_trivial("and", n))
    return _ListOperands(wah, pool, n), pool


@pytest.mark.parametrize("k", sw.LIST_OPERAND_COUNTS)
def test_list_operand_counts(wah, k):
    """Tables of 1, 2, 63, 64, 65, 127, 128, 129 and 4097 rows (the rows of a small pool in turn: a row is 24 bytes)."""
    ops, pool = _pool_operands(wah, 303)
    rows = sw.list_table_rows(k, len(pool) - 1)
    for op in sw.LIST_OPS:
        ops.check(op, rows, sw.list_fold(op, pool, rows), f"{k} rows")


@pytest.mark.parametrize("name", list(sw.LIST_PLACED))
def test_list_operand_positions(wah, name):
    """LIST_PLACED: every row but the placed ones is the operation's trivial operand (settled while the chunk is gathered) -- the
    only live operand in row 0, 1, 62, 63, 64, 65, 128; live operands in rows 0, 1, 63, 64 and 128 of one table; row 0's bitmap
    again in rows 64 and 128 (ANDNOT: A and not A -- m_first is row 0's alone); live operands in lanes 62 and 63."""
    ops, pool = _pool_operands(wah, 304)
    n_rows, placed = sw.LIST_PLACED[name]
    for op in sw.LIST_OPS:
        trivial = len(pool) - 1 if op == "and" else 0
        rows = [e if e else trivial for e in sw.list_table_rows(n_rows, len(pool) - 1, placed)]
        ops.check(op, rows, sw.list_fold(op, pool, rows), name)


@pytest.mark.parametrize("tail", sw.LAST_SEGMENT_WORDS)
def test_list_ragged_ends(wah, tail):
    """A last segment of 2, 31, 32, 34, 1023 groups that is one fill of zeros (settled with count == nvalid; under AND a fill with
    an effect), one fill of ones as far as a bitmap can hold one, or literals up to the last group."""
    rng = np.random.default_rng(305 + tail)
    head = [sw.list_words_layout(130, "fill first", 1), sw.list_words_layout(1024, "literals + fill", 0)]
    ways = sw.list_ragged_layouts(tail)
    maps = [sw.list_probe_bitmap(head, rng, tail=(layout, tail)) for layout in ways.values()]
    n = maps[0].size
    maps.append(rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32))
    ops = _ListOperands(wah, maps, n)
    for op in sw.LIST_OPS:
        for rows in ([0], [1], [2], [0, 3], [3, 0], [1, 3], [3, 1], [2, 3], [3, 2, 1, 0], [0, 1, 2, 3]):
            ops.fold(op, rows, f"a last segment of {tail} words, rows {rows}")


@pytest.mark.parametrize("n_segments", sw.LIST_SEGMENTS)
def test_list_segment_counts(wah, n_segments):
    """1, 3, 4 and 5 segments (kSegDecodeWaves = 4 a workgroup: idle waves in the last one), whole and with a short last one."""
    rng = np.random.default_rng(306 + n_segments)
    for tail in (0, 30):
        maps = []
        for j in range(3):
            layouts = [sw.list_words_layout((2, 129, 1024, 300, 7)[(s + j) % 5], sw.LIST_WAYS[(s + j) % 2 * 3], (s + j) & 1) for s in range(n_segments - (1 if tail else 0))]
            maps.append(sw.list_probe_bitmap(layouts, rng, tail=(list(sw.list_ragged_layouts(tail).values())[j], tail) if tail else None))
        ops = _ListOperands(wah, maps, maps[0].size)
        for op in sw.LIST_OPS:
            ops.fold(op, [0, 1, 2], f"{n_segments} segments, tail {tail}")
            ops.fold(op, [2, 0], f"{n_segments} segments, tail {tail}")


def test_list_stream_offsets(wah):
    """One operand's stream 0, 1, 2, 3 words behind a 16-byte boundary (the batches are loaded eight bytes a lane)."""
    rng = np.random.default_rng(307)
    layouts = [p[3] for p in sw.list_words_probes()][::3]
    maps = [sw.list_probe_bitmap(layouts, rng), _dense(rng, len(layouts)), sw.list_probe_bitmap(layouts[::-1], rng)]
    ops = _ListOperands(wah, maps, maps[0].size)
    for at in range(3):
        for offset in range(4):
            moved = list(ops.dev)
            moved[at] = (_at_offset(ops.cases[at].want, offset), ops.dev[at][1])
            for op in sw.LIST_OPS:
                ops.fold(op, [0, 1, 2], f"operand {at} + {offset} words", operands=moved)


def _refused(ops, operands, valid_rows, what):
    """`operands` gives WAH_ERR_STREAM under every operation, nothing is written behind the output's capacity, and the valid rows
    give the right words on the same scratch afterwards."""
    capacity = ops.wah.max_compressed_words(ops.n)
    for op in sw.LIST_OPS:
        status, _, buf, out, _ = ops.enqueue(op, operands, capacity)
        assert status == WAH_ERR_STREAM, (what, op, status)
        assert _untouched(buf, out, capacity), f"{what} [{op}]: written behind the capacity"
        ops.fold(op, valid_rows, f"after {what}", many=False)


def test_list_refusals_at_the_boundaries(wah):
    """Hand-built words that the kernel must refuse (tests/_switch.py list_refusals: 1023 and 1025 groups with the fill in batch
    1, 2 and 8; counts of 2047, 2048, 2049 and 2^30 - 1, 128 of them; an empty fill in lane 63's second word and in a later
    batch; a batch of literals behind 897 groups; a lone literal), as a later operand and as the first.  Every stream has its
    OWN index, every range inside it: these check a verdict, whatever the kernel does it reads allocated memory only."""
    import torch

    rng = np.random.default_rng(308)
    ops, pool = _pool_operands(wah, 308)
    oracle = _oracle.load()
    valid = [oracle.compress(pool[2][lo: lo + sw.SEG_WORDS]) for lo in range(0, ops.n, sw.SEG_WORDS)]
    for name, words in sw.list_refusals(rng):
        for segment in (1, 2):
            stream, index = sw.list_refused_stream(valid, segment, words)
            bad = (_dev(stream), torch.from_numpy(index).cuda())
            _refused(ops, [ops.dev[1], bad, ops.dev[3]], [1, 3], f"{name} (segment {segment}, row 1)")
        _refused(ops, [bad, ops.dev[1]], [2, 1], f"{name} (row 0)")
        _refused(ops, [bad], [2], f"{name} (alone)")


@pytest.mark.parametrize("tail", [30, 991])
def test_list_refused_identity_fill_of_another_length(wah, tail):
    """The settled path's own check (count == nvalid): as an operand, the all-zero stream of a bitmap one word shorter and one
    longer with as many segments -- its last segment is ONE identity fill of nvalid - 1 and of nvalid + 1 groups."""
    import torch

    rng = np.random.default_rng(309)
    n = sw.SEG_WORDS + tail
    maps = [rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32), np.zeros(n, np.uint32)]
    ops = _ListOperands(wah, maps, n)
    nvalid = (32 * tail + 30) // 31
    for other, d in ((n - 1, -1), (n + 1, 1)):
        zero = _Case("zeros", np.zeros(other, np.uint32))
        assert list(zero.want) == [sw.FILL0 | sw.SEG_GROUPS, sw.FILL0 | (nvalid + d)] and list(zero.index) == [0, 1, 2]
        bad = (_dev(zero.want), torch.from_numpy(zero.index).cuda())
        for operands in ([ops.dev[0], bad], [bad, ops.dev[0]], [bad], [ops.dev[0], ops.dev[1], bad]):
            _refused(ops, operands, [0, 1], f"an identity fill of nvalid {d:+d} groups among {len(operands)}")


@pytest.mark.parametrize("k, row", [(sw.LIST_CHUNK, sw.LIST_CHUNK - 1), (sw.LIST_CHUNK + 1, sw.LIST_CHUNK), (4097, 4096)])
def test_list_refused_rows(wah, k, row):
    """A bad entry in row 63, in row 64 only, and in the last of 4097 rows: an operand whose one segment has 1025 groups, and a
    table entry without an index."""
    import torch

    rng = np.random.default_rng(310)
    ops, pool = _pool_operands(wah, 310)
    oracle = _oracle.load()
    valid = [oracle.compress(pool[2][lo: lo + sw.SEG_WORDS]) for lo in range(0, ops.n, sw.SEG_WORDS)]
    name, words = sw.list_refusals(rng)[1]
    assert name.startswith("1025 groups")
    stream, index = sw.list_refused_stream(valid, 2, words)
    bad = (_dev(stream), torch.from_numpy(index).cuda())
    rows = sw.list_table_rows(k, len(pool) - 1)
    operands = [ops.dev[i] for i in rows]
    operands[row] = bad
    _refused(ops, operands, rows[:3], f"{name} in row {row} of {k}")
    table = wah.bitop_operand_table([ops.dev[i] for i in rows])
    table[row, 2] = 0
    _refused(ops, table, rows[:3], f"no index in row {row} of {k}")

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

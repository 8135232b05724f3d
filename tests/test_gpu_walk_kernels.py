"""GPU tests: the stream checker, the index builder and the fill merger (the tiled walk of wah_aux.hip) on the edges of their
tiles, threads and waves, of the merge scan's rounds of 1024 tiles and of the 2^29-group blocks.

tests/_walk.py builds the streams and the vectorised references (tests/test_walk_reference.py proves both on the CPU).  Every
stream goes through wah_validate_device, wah_merge_fills_device and wah_build_index_device -- the C entry points, so that
every output lies in a buffer of exactly its size with a sentinel behind it -- at four placements: 0, 4, 8 and 12 bytes behind
a 16-byte boundary (only placement 0 takes the 16-byte tile loads, and only for whole tiles).  Checked on every run: the exact
report, the exact merged words and their count, the exact index and [words, groups], WAH_ERR_STREAM exactly where the
reference refuses the index, the sentinel behind every output, and the input (with the words in front of it and behind it,
which would move every counter if they were read) unchanged.

Device decodes of merged streams are capped at DECODE_CAP_WORDS decoded words (16 MiB): every run probe is far below it, the
2^29 probes (up to 2^32 groups and more) are above and are checked by their words only.

That the tests bite: libraries with ONE token of wah_aux.hip changed (only values that are compared, counted or summed), this
file run once against each on an MI355X.  [family] = test_edge_probes_at_every_placement[family], rounds =
test_more_than_one_round_of_the_merge_scan, capacities and merged = the last two tests.

  thread 0's prev from global memory -> 0u            [pairs] [runs], rounds (the four streams with a run), merged
  k < wave -> k <= wave, checker's position sum       every test but capacities
    ... index builder's                               [pairs] [positions] [ends] [index] [runs], capacities
    ... merger's                                      every test
  > kSegGroups -> >=, checker                         every test but capacities
    ... index builder                                 [pairs] [positions] [index], capacities
  unmerged rule without `(p & 1023) != 0`             [pairs] [positions] [index] [runs] [blocks], four of rounds, merged
  unmerged rule without `(prev & kCountMask) != 0`    [pairs] [runs]
  cnt - 1u -> cnt in merge_dropped                    [blocks], merged
  kMergeBlockShift 29 -> 28                           [blocks], merged
  k = wave + 1 -> k = wave, scatter's suffix minimum  every test
    ... the scan's                                    every test
  s_carry not updated, forward loop                   every test (the total itself comes through it)
    ... backward loop                                 rounds: the four streams whose run crosses a round
  have_prev = w0 > 0 -> true (checker; merger)        NOT caught, and cannot be: tests/_switch.py says why

Not built: `!= 0u` alone dropped from the unmerged rule (each term keeps its truth value: the same program); `& 15u` -> `& 3u`
(it would issue 16-byte loads from addresses that are only 4-byte aligned; every stream of whole tiles here runs at placements
4, 8 and 12 and must give what placement 0 gives, and tests/test_switch_reference.py reads the 15 out of the source).
"""
import numpy as np
import pytest

from tests import _walk as wk
from tests.test_gpu_parity import _dev, _host, wah  # noqa: F401 (wah: the fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A
GUARD = 64                      # entries behind every output that must keep the sentinel
WAH_ERR_CAPACITY = -4
WAH_ERR_STREAM = -6
DECODE_CAP_WORDS = 1 << 22


class _Placed:
    """A stream in device memory, `byte` bytes behind a 16-byte boundary: fills in front of it, wk.PADDING behind it."""

    def __init__(self, stream, byte):
        front = byte // 4
        self.c = int(stream.size)
        self.host = np.concatenate([np.full(front, wk.FILL1 | 5, np.uint32), stream, wk.PADDING])
        self.buf = _dev(self.host)
        self.d = self.buf[front: front + self.c]
        assert self.d.data_ptr() % 16 == byte, (self.d.data_ptr(), byte)

    def unchanged(self):
        return np.array_equal(_host(self.buf), self.host)


def _full(n, value, dtype):
    import torch

    return torch.full((n, ), value, dtype=dtype, device="cuda")


def _zeros(n_bytes):
    import torch

    return torch.zeros(max(int(n_bytes), 1), dtype=torch.uint8, device="cuda")


def _validate(lib, placed):
    """(status, the report's eight entries, the sentinel behind them is intact)."""
    import torch

    ws_bytes = int(lib.wah_decompress_workspace_bytes(placed.c, 0))
    ws = _zeros(ws_bytes)
    rep = _full(8 + GUARD, SENTINEL64, torch.int64)
    assert lib.wah_validate_device(placed.d.data_ptr(), placed.c, rep.data_ptr(), ws.data_ptr(), ws_bytes, None) == 0, lib.wah_last_error()
    status = int(lib.wah_decompress_status(ws.data_ptr(), None))
    r = rep.cpu().tolist()
    return status, r[:8], all(v == SENTINEL64 for v in r[8:])


def _merge(lib, placed, capacity):
    """(status, the count, the output's `capacity` words as they are, the sentinel behind them and the count is intact)."""
    import torch

    ws_bytes = int(lib.wah_merge_fills_workspace_bytes(placed.c))
    ws = _zeros(ws_bytes)
    out = _full(capacity + GUARD, SENTINEL, torch.int32)
    count = _full(1 + GUARD, SENTINEL64, torch.int64)
    assert lib.wah_merge_fills_device(placed.d.data_ptr(), placed.c, out.data_ptr(), capacity, count.data_ptr(), ws.data_ptr(), ws_bytes,
                                      None) == 0, lib.wah_last_error()
    status = int(lib.wah_decompress_status(ws.data_ptr(), None))
    intact = bool((out[capacity:] == SENTINEL).all()) and bool((count[1:] == SENTINEL64).all())
    return status, int(count[0].item()), out[:capacity], intact


def _build_index(lib, placed, capacity, room=None):
    """(status, [words, groups], the buffer of `room` entries (default: capacity) + GUARD as it is, the info's sentinel is intact)."""
    import torch

    room = capacity if room is None else room
    ws_bytes = int(lib.wah_decompress_workspace_bytes(placed.c, 0))
    ws = _zeros(ws_bytes)
    offs = _full(room + GUARD, SENTINEL64, torch.int64)
    info = _full(2 + GUARD, SENTINEL64, torch.int64)
    assert lib.wah_build_index_device(placed.d.data_ptr(), placed.c, offs.data_ptr(), capacity, info.data_ptr(), ws.data_ptr(), ws_bytes,
                                      None) == 0, lib.wah_last_error()
    status = int(lib.wah_decompress_status(ws.data_ptr(), None))
    return status, info[:2].tolist(), offs, bool((info[2:] == SENTINEL64).all())


def _check_all_three(wah, probe, bytes_behind=wk.PLACEMENT_BYTES):
    """The probe through the three calls at every placement, against the references; returns the merged words (device, from
    the last placement)."""
    lib = wah.lib()
    st = probe.stream
    want_report, want_merged, want_index = wk.report(st), wk.merged(st), wk.index(st)
    refused = isinstance(want_index, str)
    entries = wk.segments_of(st) + 1
    merged_dev = None
    for byte in bytes_behind:
        what = f"{probe.name} [{byte} bytes behind a 16-byte boundary]"
        placed = _Placed(st, byte)
        status, r, intact = _validate(lib, placed)
        assert status == 0 and intact, (what, status)
        assert tuple(r[:6]) + (bool(r[6]), ) == want_report and r[6] in (0, 1) and r[7] == 0, (what, r, want_report)
        status, count, out, intact = _merge(lib, placed, int(want_merged.size))
        assert status == 0 and count == want_merged.size and intact, (what, status, count, want_merged.size)
        got = _host(out)
        assert np.array_equal(got, want_merged), (what, np.flatnonzero(got != want_merged)[:5])
        merged_dev = out
        status, info, offs, intact = _build_index(lib, placed, entries)
        assert info == [want_report[1], want_report[0]] and intact, (what, info)
        assert bool((offs[entries:] == SENTINEL64).all()), (what, "written behind the index")
        if refused:
            assert status == WAH_ERR_STREAM, (what, status, want_index)
        else:
            assert status == 0, (what, status)
            got = offs[:entries].cpu().numpy()
            assert np.array_equal(got, want_index), (what, np.flatnonzero(got != want_index)[:5])
        if "crossing" in probe.facts:       # the 1024 - q fill is accepted, its 1025 - q neighbour refused
            assert (status == WAH_ERR_STREAM) == probe.facts["crossing"] and (r[4] == 1) == probe.facts["crossing"], what
        if "refused" in probe.facts:
            assert (status == WAH_ERR_STREAM) == probe.facts["refused"], what
        assert placed.unchanged(), (what, "the input was written to")
    return merged_dev


@pytest.fixture(scope="module")
def probes():
    return wk.small_probes()


@pytest.mark.parametrize("family", ["pairs", "positions", "ends", "index", "runs", "blocks"])
def test_edge_probes_at_every_placement(wah, probes, family):
    """pairs: the predecessor from the same thread, from LDS and from global memory; positions: the wave scan, the sums of the
    waves in front and the tile base, on both sides of the segment's end; ends: the last tile's bounds; index: segments that
    begin on every edge, and their refused neighbours; runs: threads, waves and tiles that keep nothing; blocks: the 2^29 rule,
    at 2^29 and beyond 2^32 groups."""
    assert len(probes[family]) >= 12
    for p in probes[family]:
        _check_all_three(wah, p)


@pytest.mark.parametrize("name", list(wk.SCAN_ROUND_STREAMS))
def test_more_than_one_round_of_the_merge_scan(wah, name):
    """Streams of 1023 to 2049 tiles: merge_scan_kernel's second and third round -- the carry of kept words forwards, the carry
    of first kept positions backwards (a kept fill in tile 1000 whose run ends in tile 1030; a run across a whole round that
    keeps nothing) -- and the checker and the index builder at those sizes.  The merged stream goes back through the checker."""
    p = wk.scan_round_stream(name)
    merged = _check_all_three(wah, p)
    want = wk.merged(p.stream)
    assert tuple(wah.validate_device(merged.contiguous())) == wk.report(want)
    if p.facts["run"] is not None:
        lo, hi = p.facts["run"]
        at = lo - int(np.count_nonzero(wk.dropped(p.stream)[:lo]))
        count = int((p.stream[lo: hi] & wk.COUNT_MASK).astype(np.uint64).sum())
        assert int(_host(merged[at: at + 1])[0]) == (int(p.stream[lo]) & wk.FILL1) | count


def test_capacities_exactly_at_and_one_below(wah, probes):
    """wah_merge_fills_device into exactly its words: WAH_OK (every run above does that); into one word less: WAH_ERR_CAPACITY, and
    the word behind the capacity keeps the sentinel.  wah_build_index_device with n_seg + 1 entries: WAH_OK (every run above); with
    n_seg: WAH_ERR_CAPACITY, and nothing is written at entry n_seg or behind it."""
    lib = wah.lib()
    # streams without an index (the merge's capacity; the index call says WAH_ERR_STREAM whatever its capacity), and every
    # accepted stream of the index and position families: segments that begin on every edge, entry n_seg next to them
    chosen = ([p for p in probes["runs"] if p.facts["head_count"]] + [p for p in probes["ends"] if p.facts["c_words"] > wk.TILE][:4]
              + [p for p in probes["index"] + probes["positions"] if isinstance(wk.index(p.stream), np.ndarray)])
    indexed = [p for p in chosen if isinstance(wk.index(p.stream), np.ndarray)]
    assert len(indexed) >= 2 + len(wk.WALK_EDGES) * (1 + len(wk.POSITION_Q)) and len(chosen) - len(indexed) >= 10
    for p in chosen:
        st = p.stream
        total, n_seg = int(wk.merged(st).size), wk.segments_of(st)
        assert total >= 2 and n_seg >= 1
        for byte in wk.PLACEMENT_BYTES:
            what = f"{p.name} [{byte} bytes behind a 16-byte boundary]"
            placed = _Placed(st, byte)
            status, count, out, intact = _merge(lib, placed, total - 1)
            assert status == WAH_ERR_CAPACITY and intact, (what, status)           # (intact: the word at total - 1 and GUARD - 1 more)
            status, info, offs, intact = _build_index(lib, placed, n_seg, room=n_seg + 1)
            expect = WAH_ERR_STREAM if isinstance(wk.index(st), str) else WAH_ERR_CAPACITY
            assert status == expect and intact, (what, status)
            assert bool((offs[n_seg:] == SENTINEL64).all()), (what, "written at or behind entry n_seg")
            if expect == WAH_ERR_CAPACITY:                                         # the entries that fit are the index's
                assert np.array_equal(offs[:n_seg].cpu().numpy(), wk.index(st)[:n_seg]), what
            assert placed.unchanged(), what


def test_merged_streams_validate_and_decode(wah, probes):
    """The merged form of the run probes and of the 2^29 probes goes back through the checker (its report: the reference's on
    the merged words); the run probes' is decoded on the device as well and equals the decode of the original."""
    for family in ("runs", "blocks"):
        for p in probes[family]:
            st = p.stream
            want = wk.merged(st)
            merged = wah.merge_fills_device(_dev(st))
            assert np.array_equal(_host(merged), want), p.name
            if want.size:
                rep = wk.report(want)
                assert tuple(wah.validate_device(merged)) == rep, p.name
                assert rep[0] == wk.groups(st) and rep[2] == 0, p.name
            words = (31 * wk.groups(st) + 31) // 32
            if family == "runs":
                assert words <= DECODE_CAP_WORDS, p.name
                if want.size:
                    a = _host(wah.decompress_device(merged, words + 2))
                    b = _host(wah.decompress_device(_dev(st), words + 2))
                    assert a.size == words and np.array_equal(a, b), p.name
            else:
                assert words > DECODE_CAP_WORDS   # by words only

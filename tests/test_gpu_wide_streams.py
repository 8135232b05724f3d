"""GPU tests: streams that decode beyond 32-bit group counts, through every decoder route.

The decoder switches between 32-bit and 64-bit code at 2^31 / 2^32 groups per tile and per stream; the streams here reach
those counts cheaply -- a few thousand fill words of 2^20 to 2^25 groups, ordinary data in front of them and behind them
(tests/_wide.py builds them and checks the multi-GB outputs piece by piece on the device).  One output buffer serves every
case (the largest output, C4, is about 25 GB); it is refilled with a sentinel before every decode, so that a route that
writes nothing cannot pass on what an earlier route left.
"""
import functools

import numpy as np
import pytest

from tests import _oracle, _wide
from tests.test_gpu_parity import _dev, _host, _py_merge_fills, _py_report, _route_is, wah  # noqa: F401 (wah: the fixture)

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 4096  # words behind the capacity that must keep the sentinel
WAH_ERR_STREAM = -6

# route -> the decoder wah_last_decode_route() must report (1 one pass, 2 two launches, 3 no wait)
ROUTES = {"default": 1, "one pass": 1, "two launches": 2, "no wait": 3, "4-byte aligned": 2, "scan + expand": 2}
FLAGS = {"one pass": 8, "two launches": 4, "no wait": 2}


@functools.lru_cache(maxsize=None)
def _case(case):
    return _wide.giant_case(_oracle.load(), case)


@pytest.fixture(scope="module")
def out_buffer(wah):
    """One output buffer for every case of the module: the largest output + the guard."""
    import torch

    words = max(_case(c).words for c in _wide.GIANT_CASES)
    buf = torch.empty(words + GUARD, dtype=torch.int32, device="cuda")
    yield buf
    del buf
    torch.cuda.empty_cache()


class _Decoder:
    """The stream of a case on the device (16-byte aligned, or `offset` words behind such a boundary; and a copy that is only
    4-byte aligned), a workspace for the exact capacity, the info words."""

    def __init__(self, wah, stream, capacity, offset=0):
        import torch

        self.lib = wah.lib()
        self.c = int(stream.size)
        self.cap = int(capacity)
        self.d_buf = _dev(np.concatenate([np.zeros(offset, np.uint32), stream]))
        self.d = self.d_buf[offset:]
        self.d_odd_buf = _dev(np.concatenate([np.zeros(1, np.uint32), stream]))
        self.d_odd = self.d_odd_buf[1:]
        assert self.d.data_ptr() % 16 == 4 * offset and self.d_odd.data_ptr() % 16 == 4
        self.ws_bytes = int(self.lib.wah_decompress_workspace_bytes(self.c, self.cap))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device="cuda")
        self.info = torch.zeros(2, dtype=torch.int64, device="cuda")

    def status(self):
        return int(self.lib.wah_decompress_status(self.ws.data_ptr(), None))

    def error(self):
        return self.lib.wah_last_error().decode()

    def run(self, route, out):
        """Decode by `route` into out (capacity self.cap); returns (status, the route the library reports, info)."""
        lib, ws, info = self.lib, self.ws.data_ptr(), self.info.data_ptr()
        self.info.fill_(-1)
        if route == "scan + expand":
            rc = lib.wah_decompress_scan_device(self.d.data_ptr(), self.c, info, ws, self.ws_bytes, None)
            assert rc == 0, (route, rc, self.error())
            seen = int(lib.wah_last_decode_route())  # (the expand call alone has no sums pass to choose a route for)
            st = self.status()
            if st != 0:
                return st, seen, self.info.tolist()
            rc = lib.wah_decompress_expand_device(self.d.data_ptr(), self.c, out.data_ptr(), self.cap, info, ws, self.ws_bytes, None)
        elif route in ("default", "4-byte aligned"):
            d = self.d if route == "default" else self.d_odd
            rc = lib.wah_decompress_device(d.data_ptr(), self.c, out.data_ptr(), self.cap, info, ws, self.ws_bytes, None)
            seen = int(lib.wah_last_decode_route())
        else:
            rc = lib.wah_decompress_device_ex(self.d.data_ptr(), self.c, out.data_ptr(), self.cap, info, FLAGS[route], ws,
                                              self.ws_bytes, None)
            seen = int(lib.wah_last_decode_route())
        assert rc == 0, (route, rc, self.error())
        return self.status(), seen, self.info.tolist()


@functools.lru_cache(maxsize=None)
def _decoder(case):
    import importlib

    ws = _case(case)
    return _Decoder(importlib.import_module("gpu-wah_amd"), ws.stream(), ws.words)


def _decode_and_check(ws, dec, route, out_buffer):
    words, groups = ws.expected()
    assert dec.cap == words
    view = out_buffer[: words + GUARD]
    view.fill_(SENTINEL)
    status, seen, info = dec.run(route, view[:words])
    assert status == 0, f"{ws.name} [{route}]: status {status} ({dec.error()})"
    assert _route_is(seen, ROUTES[route]), (ws.name, route, seen)
    assert info == [words, groups], (ws.name, route, info)
    ws.check(view[:words], f" [{route}]")
    assert bool((view[words:] == SENTINEL).all()), f"{ws.name} [{route}]: written behind the capacity"


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("case", _wide.GIANT_CASES)
def test_wide_stream_decodes_on_every_route(wah, out_buffer, case, route):
    """C1 tame tile (< 2^31 groups), C2 partial staging above 2^31, C3 exactly 2^32 in one tile, C4 2^32 + 2^31 with a bucket
    of 2^31 and data beyond 2^32 output words, C5 a saturated bucket (control), C6 the giant fills across a one-pass tile's
    end (tests/_wide.py: giant_case): status, every output word, nothing behind the capacity, info, the route."""
    _decode_and_check(_case(case), _decoder(case), route, out_buffer)


@pytest.mark.parametrize("case", _wide.GIANT_CASES)
def test_wide_stream_checks_without_expanding(wah, case):
    """The stream-level calls on the same streams: the checker's report, the merged form, and no segment index (the giant
    fills cross segments)."""
    import torch

    ws = _case(case)
    st = ws.stream()
    dec = _decoder(case)
    assert tuple(wah.validate_device(dec.d)) == _py_report(st)
    assert np.array_equal(_host(wah.merge_fills_device(dec.d)), _py_merge_fills(st))
    lib = wah.lib()
    entries = (ws.groups + 1023) // 1024 + 1  # (room enough: the refusal is about the stream, not the capacity)
    offsets = torch.zeros(entries, dtype=torch.int64, device="cuda")
    info = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws_bytes = int(lib.wah_decompress_workspace_bytes(dec.c, 0))
    work = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
    assert lib.wah_build_index_device(dec.d.data_ptr(), dec.c, offsets.data_ptr(), entries, info.data_ptr(), work.data_ptr(),
                                      ws_bytes, None) == 0
    assert lib.wah_decompress_status(work.data_ptr(), None) == WAH_ERR_STREAM


def test_merged_wide_stream_beyond_2_32(wah, out_buffer):
    """C4's fills come in runs of one kind: merged (classic unsegmented WAH), runs join and are cut at multiples of 2^29 groups
    beyond 2^32, and the fills exceed 2^25 -- saturated buckets at high bases.  The merged stream decodes to C4's bitmap."""
    ws = _case("C4")
    st = ws.stream()
    merged = wah.merge_fills_device(_dev(st))
    want = _py_merge_fills(st)
    assert np.array_equal(_host(merged), want)
    # cuts of the 2^29 rule beyond 2^32: two neighbouring fills of one kind in the merged stream (anything else is merged)
    pos, cuts, longest = 0, 0, 0
    prev = None
    for x in (int(v) for v in want):
        n = x & 0x3FFFFFFF if x & 0x80000000 else 1
        if prev is not None and x & 0x80000000 and prev & 0x80000000 and not (x ^ prev) & 0x40000000 and pos > 1 << 32:
            cuts += 1
        if x & 0x80000000:
            longest = max(longest, n)
        pos += n
        prev = x
    assert pos == ws.groups and cuts >= 2 and longest > 1 << 25, (cuts, longest)
    assert tuple(wah.validate_device(merged)) == _py_report(want)
    dec = _Decoder(wah, want, ws.words)
    _decode_and_check(ws, dec, "default", out_buffer)


@pytest.mark.parametrize("forced", [False, True])
def test_sums_pass_limit_of_2_47_groups(wah, monkeypatch, forced):
    """kSumSaturate: 131 072 fills of 2^30 - 32 groups (2^47 - 2^22) are counted exactly by wah_decompress_scan_device, on the
    normal route and on the no-wait route; one more fill reaches 2^47 and is reported, never WAH_OK.  Nothing is expanded."""
    import torch

    if forced:
        monkeypatch.setenv("WAH_FORCE_FALLBACK", "1")
    lib = wah.lib()
    for extra in (0, 1):
        st, (words, groups) = _wide.sum_limit_stream(extra)
        d = _dev(st)
        ws_bytes = int(lib.wah_decompress_workspace_bytes(st.size, 0))
        work = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        info = torch.zeros(2, dtype=torch.int64, device="cuda")
        assert lib.wah_decompress_scan_device(d.data_ptr(), st.size, info.data_ptr(), work.data_ptr(), ws_bytes, None) == 0
        assert _route_is(lib.wah_last_decode_route(), 3 if forced else 2)
        status = lib.wah_decompress_status(work.data_ptr(), None)
        if extra == 0:
            assert groups == (1 << 47) - (1 << 22)
            assert status == 0 and info.tolist() == [words, groups], (status, info.tolist())
        else:
            assert groups >= 1 << 47
            assert status == WAH_ERR_STREAM, status

"""ctypes binding of libwah_hip.so (C ABI: include/wah.h).

PyTorch is used only as plumbing for device memory and streams in the
device-pointer helpers; no torch type crosses the ABI (plain pointers, sizes
and a hipStream_t passed as void*).
"""
import collections
import ctypes
import os
import subprocess
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# WAH_LIB_PATH selects another build of the same library (tools/ use it for the diagnostic build)
_LIB_PATH = os.environ.get("WAH_LIB_PATH") or os.path.join(_HERE, "libwah_hip.so")

Timings = collections.namedtuple("Timings", "to_device_ms device_ms from_device_ms")

_u32p = ctypes.POINTER(ctypes.c_uint32)
_u64p = ctypes.POINTER(ctypes.c_uint64)
_f32p = ctypes.POINTER(ctypes.c_float)
_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
_sz = ctypes.c_size_t
_int = ctypes.c_int

# name -> (restype, argtypes): every extern "C" symbol include/wah.h declares
ABI_SYMBOLS = {
    "wah_compress": (_vp, [_vp, _u64, _u64p, _f32p, _f32p, _f32p]),
    "wah_decompress": (_vp, [_vp, _u64, _u64p, _f32p, _f32p, _f32p]),
    "wah_free": (None, [_vp]),
    "wah_host_cache_release": (None, []),
    "wah_max_compressed_words": (_u64, [_u64]),
    "wah_decoded_words": (_u64, [_u64]),
    "wah_compress_workspace_bytes": (_sz, [_u64]),
    "wah_decompress_workspace_bytes": (_sz, [_u64, _u64]),
    "wah_workspace_init_device": (_int, [_vp, _sz, _vp]),
    "wah_compress_device": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_compress_device_ex": (_int, [_vp, _u64, _vp, _u64, _vp, ctypes.c_uint, _vp, _sz, _vp]),
    "wah_compress_device_indexed": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_compress_status": (_int, [_vp, _vp]),
    "wah_compress_columns_multi_device": (_int, [_int, _vp, _u64, _vp]),
    "wah_decompress_device": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_decompress_device_ex": (_int, [_vp, _u64, _vp, _u64, _vp, ctypes.c_uint, _vp, _sz, _vp]),
    "wah_decompress_scan_device": (_int, [_vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_decompress_expand_device": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_build_index_device": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_decompress_segments_workspace_bytes": (_sz, []),
    "wah_decompress_segments_device": (ctypes.c_int, [_vp, _u64, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _sz, _vp]),
    "wah_decompress_status": (_int, [_vp, _vp]),
    "wah_validate_device": (_int, [_vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_merge_fills_workspace_bytes": (_sz, [_u64]),
    "wah_merge_fills_device": (_int, [_vp, _u64, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_bitop_scratch_bytes": (_sz, [_u64, _u64, _u64]),
    "wah_bitop_device": (_int, [_int, _u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_bitop_status": (_int, [_vp, _u64, _u64, _u64, _vp]),
    "wah_bitop_indexed_scratch_bytes": (_sz, [_u64]),
    "wah_bitop_indexed_device": (_int, [_int, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bitop_indexed_status": (_int, [_vp, _u64, _vp]),
    "wah_bitop_many_indexed_device": (_int, [_int, _u64, _int, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bitop_list_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_bitop_list_indexed_device": (_int, [_int, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bitop_list_status": (_int, [_vp, _u64, _u64, _vp]),
    "wah_bitop_clauses_scratch_bytes": (_sz, [_u64, _u64, _u64]),
    "wah_bitop_clauses_indexed_device": (_int, [_u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bitop_clauses_status": (_int, [_vp, _u64, _u64, _u64, _vp]),
    "wah_bsi_range_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_bsi_range_indexed_device": (_int, [_u64, _u64, _vp, _vp, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_range_status": (_int, [_vp, _u64, _u64, _vp]),
    "wah_bsi_member_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_bsi_member_indexed_device": (_int, [_u64, _u64, _vp, _vp, _u64, _vp, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_member_status": (_int, [_vp, _u64, _u64, _vp]),
    "wah_bsi_compare_scratch_bytes": (_sz, [_u64, _u64, _u64]),
    "wah_bsi_compare_indexed_device": (_int, [_int, _u64, _u64, _u64, _vp, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_compare_status": (_int, [_vp, _u64, _u64, _u64, _vp]),
    "wah_bsi_arith_scratch_bytes": (_sz, [_u64, _u64, ctypes.c_uint]),
    "wah_bsi_arith_indexed_device": (_int, [_int, _u64, _u64, _u64, _u64, _vp, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_arith_status": (_int, [_vp, _u64, _u64, ctypes.c_uint, _vp]),
    "wah_bsi_mul_scratch_bytes": (_sz, [_u64, _u64, _u64, ctypes.c_uint]),
    "wah_bsi_mul_indexed_device": (_int, [_u64, _u64, _u64, _u64, _vp, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_mul_status": (_int, [_vp, _u64, _u64, _u64, ctypes.c_uint, _vp]),
    "wah_bsi_div_scratch_bytes": (_sz, [_u64, _u64, _u64, ctypes.c_uint]),
    "wah_bsi_div_indexed_device": (_int, [_int, _u64, _u64, _u64, _u64, _vp, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_div_status": (_int, [_vp, _u64, _u64, _u64, ctypes.c_uint, _vp]),
    "wah_bsi_kth_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_bsi_kth_indexed_device": (_int, [_u64, _u64, _u64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_kth_status": (_int, [_vp, _vp]),
    "wah_bsi_kth_grouped_scratch_bytes": (_sz, [_u64, _u64, _u64, _u64]),
    "wah_bsi_kth_grouped_indexed_device": (_int, [_u64, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_kth_grouped_status": (_int, [_vp, _vp]),
    "wah_fetch_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_fetch_indexed_device": (_int, [ctypes.c_uint, _u64, _u64, _vp, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_fetch_status": (_int, [_vp, _vp]),
    "wah_values_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_values_indexed_device": (_int, [ctypes.c_uint, _u64, _u64, _vp, _u64, _u64, _vp, _vp, _sz, _vp]),
    "wah_values_status": (_int, [_vp, _vp]),
    "wah_select_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_count_list_indexed_device": (_int, [_u64, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_count_masked_indexed_device": (_int, [_u64, _u64, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_group_sum_indexed_device": (_int, [_u64, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "wah_positions_indexed_device": (_int, [_u64, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _sz, _vp]),
    "wah_select_status": (_int, [_vp, _vp]),
    "wah_bsi_group_by_scratch_bytes": (_sz, [_u64]),
    "wah_bsi_group_by_indexed_device": (_int, [_u64, _u64, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _u64, ctypes.c_uint, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_group_by_status": (_int, [_vp, _vp]),
    "wah_bsi_map_scratch_bytes": (_sz, [_u64, _u64, ctypes.c_uint]),
    "wah_bsi_map_indexed_device": (_int, [_u64, _u64, _u64, _vp, _vp, _u64, _u64, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_map_status": (_int, [_vp, _u64, _u64, ctypes.c_uint, _vp]),
    "wah_bsi_cumsum_scratch_bytes": (_sz, [_u64, _u64, ctypes.c_uint]),
    "wah_bsi_cumsum_indexed_device": (_int, [_u64, _u64, _u64, _vp, _u64, _vp, _u64, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_cumsum_status": (_int, [_vp, _u64, _u64, ctypes.c_uint, _vp]),
    "wah_bsi_cumsum_parts_scratch_bytes": (_sz, [_u64, _u64, ctypes.c_uint]),
    "wah_bsi_cumsum_parts_indexed_device": (_int, [_u64, _u64, _u64, _vp, _u64, _vp, _vp, _u64, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_cumsum_parts_status": (_int, [_vp, _u64, _u64, ctypes.c_uint, _vp]),
    "wah_bsi_total_parts_scratch_bytes": (_sz, [_u64, _u64, ctypes.c_uint]),
    "wah_bsi_total_parts_indexed_device": (_int, [_u64, _u64, _u64, _vp, _u64, _vp, _vp, _u64, ctypes.c_uint, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_total_parts_status": (_int, [_vp, _u64, _u64, ctypes.c_uint, _vp]),
    "wah_from_positions_max_words": (_u64, [_u64, _u64, _u64]),
    "wah_from_positions_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_from_positions_device": (_int, [_u64, _u64, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_from_positions_status": (_int, [_vp, _vp]),
    "wah_splice_max_words": (_u64, [_u64, _u64, _u64, _u64]),
    "wah_splice_scratch_bytes": (_sz, [_u64, _u64, _u64]),
    "wah_splice_indexed_device": (_int, [_u64, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_splice_status": (_int, [_vp, _vp]),
    "wah_compact_max_words": (_u64, [_u64, _u64, _u64]),
    "wah_compact_scratch_bytes": (_sz, [_u64, _u64, _u64]),
    "wah_compact_indexed_device": (_int, [_u64, _u64, ctypes.c_uint32, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "wah_compact_status": (_int, [_vp, _vp]),
    "wah_update_max_words": (_u64, [_u64, _u64, _u64, _u64]),
    "wah_update_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_update_indexed_device": (_int, [_u64, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_update_status": (_int, [_vp, _vp]),
    "wah_bsi_build_scratch_bytes": (_sz, [_u64, _u64]),
    "wah_bsi_build_device": (_int, [_u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _sz, _vp]),
    "wah_bsi_build_status": (_int, [_vp, _u64, _u64, _vp]),
    "wah_gen_uniform_device": (_int, [_vp, _u64, _u64, _u64, _vp]),
    "wah_gen_clustered_device": (_int, [_vp, _u64, _u64, _u64, _vp]),
    "wah_copy_device": (_int, [_vp, _vp, _u64, _vp]),
    "wah_last_decode_route": (_int, []),
    "wah_last_bitop_route": (_int, []),
    "wah_last_error": (ctypes.c_char_p, []),
    "wah_version": (ctypes.c_char_p, []),
}
# the reference's own C++-linkage symbols (compress.h:12-18, decompress.h:11-17)
CXX_SYMBOLS = ("_Z8compressPjyPyPfS1_S1_", "_Z10decompressPjyPyPfS1_S1_")


class WahError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


def build(force=False, verbose=False):
    """Compile libwah_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    srcs = [os.path.join(_HERE, "csrc", f) for f in os.listdir(os.path.join(_HERE, "csrc"))]
    srcs += [os.path.join(_HERE, "..", "include", f) for f in ("wah.h", "wah_gen.h", "compress.h", "decompress.h")]
    stale = force or not os.path.exists(_LIB_PATH) or any(
        os.path.getmtime(s) > os.path.getmtime(_LIB_PATH) for s in srcs)
    if stale:
        cmd = ["make", "-C", _HERE, "libwah_hip.so"] + (["-B"] if force else [])
        subprocess.check_call(cmd, stdout=None if verbose else subprocess.DEVNULL)
    return _LIB_PATH


_lib = None


def lib():
    """Load the HIP library; fail loudly when it is missing (there is no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise WahError(f"{_LIB_PATH} not found: build it with __graft_entry__.build() or "
                           f"`make -C {_HERE}` -- the HIP extension is required, there is no CPU fallback")
        # PyTorch-ROCm ships its own libamdhip64.so (same soname).  Import it first when it is installed, so
        # that this process has ONE HIP runtime: loading ours first makes torch map a second copy, and the
        # second runtime to initialise cannot create events or streams.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        handle = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in ABI_SYMBOLS.items():
            fn = getattr(handle, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def version():
    return lib().wah_version().decode()


def _err():
    return lib().wah_last_error().decode()


def _check(rc, what):
    if rc != 0:
        raise WahError(f"{what} failed (code {rc}): {_err()}")


def max_compressed_words(n_words):
    return int(lib().wah_max_compressed_words(int(n_words)))


def decoded_words(n_groups):
    return int(lib().wah_decoded_words(int(n_groups)))


def threshold_for(p):
    """Generator threshold for bit density p (include/wah_gen.h)."""
    return min(int(p * 2**32), 2**32)


# --------------------------------------------------------------------------
# host-pointer operators: the reference's API
# --------------------------------------------------------------------------
def _host_call(fn, data):
    a = np.ascontiguousarray(data, dtype=np.uint32)
    n_out = _u64(0)
    t = [ctypes.c_float(0.0) for _ in range(3)]
    ptr = fn(a.ctypes.data if a.size else None, a.size, ctypes.byref(n_out), ctypes.byref(t[0]), ctypes.byref(t[1]),
             ctypes.byref(t[2]))
    if not ptr:
        raise WahError(f"{fn.__name__} returned NULL: {_err()}")
    if n_out.value == 0:
        lib().wah_free(ptr)
        return np.empty(0, dtype=np.uint32), Timings(*(x.value for x in t))
    # hand the library's buffer out as it is (no second copy of up to a bitmap); freed when the array goes away
    buf = (ctypes.c_uint32 * n_out.value).from_address(ptr)
    weakref.finalize(buf, lib().wah_free, ptr)
    return np.frombuffer(buf, dtype=np.uint32), Timings(*(x.value for x in t))


def compress(data, with_timings=False):
    """compress() of the reference (compress.cu:41-209): host bitmap words in, compressed words out."""
    out, t = _host_call(lib().wah_compress, data)
    return (out, t) if with_timings else out


def decompress(comp, with_timings=False):
    """decompress() of the reference (decompress.cu:18-141): returns the ceil(31*G/32) decoded words."""
    out, t = _host_call(lib().wah_decompress, comp)
    return (out, t) if with_timings else out


# --------------------------------------------------------------------------
# device-pointer operators (torch tensors as device memory; int32 storage)
# --------------------------------------------------------------------------
def host_cache_release():
    """Return the device buffers compress()/decompress() keep between calls (include/wah.h: wah_host_cache_release)."""
    lib().wah_host_cache_release()


def _torch():
    import torch

    if not torch.cuda.is_available():
        raise WahError("no GPU visible: the device-pointer API needs an MI355X")
    return torch


def _stream_ptr(torch, stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _as_words(torch, t):
    if t.dtype not in (torch.int32, torch.uint32) or not t.is_cuda or not t.is_contiguous():
        raise WahError("expected a contiguous 32-bit integer CUDA tensor")
    return t


class DeviceCompressor:
    """Reusable workspace + output for compressing bitmaps of up to `n_words` words in HBM.

    Replaces the per-call cudaMalloc/cudaFree of compress.cu:89-103,191-193: nothing is
    allocated inside run(), so it can be timed (and graph-captured) as pure device work.
    """

    def __init__(self, n_words, device="cuda:0", indexed=False, unsegmented=False, no_wait=False):
        """no_wait: the three-launch route in which no workgroup waits for another (include/wah.h: WAH_NO_WAIT)."""
        torch = _torch()
        if indexed and unsegmented:
            raise WahError("an unsegmented stream has no segment index")
        if no_wait and indexed:
            raise WahError("the flags entry point has no index output (WAH_FORCE_FALLBACK=1 covers the indexed call)")
        self.unsegmented = bool(unsegmented)
        self.no_wait = bool(no_wait)
        self.n_words = int(n_words)
        self.capacity = max_compressed_words(self.n_words)
        self.ws_bytes = int(lib().wah_compress_workspace_bytes(self.n_words))
        # zeroed once (include/wah.h: wah_workspace_init_device); the kernel keeps it up from then on
        self.workspace = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=device)
        self.out = torch.empty(max(self.capacity, 1), dtype=torch.int32, device=device)
        self.count = torch.zeros(1, dtype=torch.int64, device=device)
        n_seg = (self.capacity + 1023) // 1024
        self.seg_offsets = torch.zeros(n_seg + 1, dtype=torch.int64, device=device) if indexed else None

    def run(self, d_in, n_words=None, stream=None, count=None):
        """Enqueue one compress pass; returns nothing (read .count / .out after synchronising).  count: another
        one-element int64 device tensor to receive C instead of .count (a slot per column, say)."""
        torch = _torch()
        _as_words(torch, d_in)
        n = self.n_words if n_words is None else int(n_words)
        if n > self.n_words or n > d_in.numel():
            raise WahError("input larger than this compressor was sized for")
        sp = _stream_ptr(torch, stream)
        if count is not None:
            if count.dtype != torch.int64 or count.numel() != 1 or not count.is_cuda:
                raise WahError("count must be a one-element int64 device tensor")
            return self._run(d_in, n, sp, count.data_ptr())
        return self._run(d_in, n, sp, self.count.data_ptr())

    def _run(self, d_in, n, sp, count_ptr):
        if self.unsegmented or self.no_wait:
            rc = lib().wah_compress_device_ex(d_in.data_ptr(), n, self.out.data_ptr(), self.capacity, count_ptr,
                                              (1 if self.unsegmented else 0) | (2 if self.no_wait else 0),
                                              self.workspace.data_ptr(), self.ws_bytes, sp)
        elif self.seg_offsets is None:
            rc = lib().wah_compress_device(d_in.data_ptr(), n, self.out.data_ptr(), self.capacity, count_ptr,
                                           self.workspace.data_ptr(), self.ws_bytes, sp)
        else:
            rc = lib().wah_compress_device_indexed(d_in.data_ptr(), n, self.out.data_ptr(), self.capacity,
                                                   count_ptr, self.seg_offsets.data_ptr(),
                                                   self.workspace.data_ptr(), self.ws_bytes, sp)
        _check(rc, "wah_compress_device")

    def status(self, stream=None):
        torch = _torch()
        _check(lib().wah_compress_status(self.workspace.data_ptr(), _stream_ptr(torch, stream)), "compress")

    def result(self, stream=None):
        """Synchronise, check the launch status, return the compressed words as a device tensor view."""
        self.status(stream)
        return self.out[: int(self.count.item())]


class DeviceDecompressor:
    """Reusable workspace + output for decoding streams of up to `c_words` words into `out_capacity` words."""

    ROUTES = {0: "none", 1: "one pass", 2: "two launches", 3: "no wait"}

    def __init__(self, c_words, out_capacity_words, device="cuda:0", no_wait=False, two_launches=False, one_pass=False):
        """no_wait: the sums pass by the route in which no workgroup waits for another (include/wah.h: WAH_NO_WAIT);
        two_launches / one_pass: that decoder whatever the capacity suggests (WAH_TWO_LAUNCHES / WAH_ONE_PASS).  After
        run(): `route` = the decoder the library launched (wah_last_decode_route)."""
        torch = _torch()
        self.no_wait = bool(no_wait)
        self.two_launches = bool(two_launches)
        self.one_pass = bool(one_pass)
        self.route = "none"
        self.c_words = int(c_words)
        self.capacity = int(out_capacity_words)
        self.ws_bytes = int(lib().wah_decompress_workspace_bytes(self.c_words, self.capacity))
        # zeroed once (include/wah.h: wah_workspace_init_device); the sums kernel keeps it up from then on
        self.workspace = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=device)
        self.out = torch.empty(max(self.capacity, 1), dtype=torch.int32, device=device)
        self.info = torch.zeros(2, dtype=torch.int64, device=device)  # [decoded words, groups]

    def run(self, d_comp, c_words=None, stream=None):
        torch = _torch()
        _as_words(torch, d_comp)
        c = self.c_words if c_words is None else int(c_words)
        if c > self.c_words or c > d_comp.numel():
            raise WahError("stream larger than this decompressor was sized for")
        rc = lib().wah_decompress_device_ex(d_comp.data_ptr(), c, self.out.data_ptr(), self.capacity, self.info.data_ptr(),
                                            (2 if self.no_wait else 0) | (4 if self.two_launches else 0) | (8 if self.one_pass else 0),
                                            self.workspace.data_ptr(), self.ws_bytes, _stream_ptr(torch, stream))
        self.route = self.ROUTES.get(int(lib().wah_last_decode_route()), "?")
        _check(rc, "wah_decompress_device")

    def status(self, stream=None):
        torch = _torch()
        _check(lib().wah_decompress_status(self.workspace.data_ptr(), _stream_ptr(torch, stream)), "decompress")

    def result(self, stream=None):
        self.status(stream)
        return self.out[: int(self.info[0].item())]


def compress_device(d_in):
    """One-shot device compress: int32 CUDA tensor in, compressed int32 CUDA tensor out."""
    c = DeviceCompressor(d_in.numel(), device=d_in.device)
    c.run(d_in)
    return c.result().clone()


def decompress_device(d_comp, out_capacity_words):
    d = DeviceDecompressor(d_comp.numel(), out_capacity_words, device=d_comp.device)
    d.run(d_comp)
    return d.result().clone()


def build_index_device(d_comp):
    """Segment index (int64 tensor, ceil(G / 1024) + 1 entries) of a stream of compress() that came without one, and its
    group count G (wah_build_index_device).  Raises for streams that have no such index."""
    torch = _torch()
    _as_words(torch, d_comp)
    c = int(d_comp.numel())
    ws_bytes = int(lib().wah_decompress_workspace_bytes(c, 0))
    workspace = torch.zeros(ws_bytes, dtype=torch.uint8, device=d_comp.device)
    info = torch.zeros(2, dtype=torch.int64, device=d_comp.device)
    # a stream of c words has at most c segments (every segment holds at least one word)
    offsets = torch.zeros(c + 1, dtype=torch.int64, device=d_comp.device)
    sp = _stream_ptr(torch)
    _check(lib().wah_build_index_device(d_comp.data_ptr(), c, offsets.data_ptr(), offsets.numel(), info.data_ptr(),
                                        workspace.data_ptr(), ws_bytes, sp), "wah_build_index_device")
    _check(lib().wah_decompress_status(workspace.data_ptr(), sp), "build_index")
    groups = int(info[1].item())
    return offsets[: (groups + 1023) // 1024 + 1].clone(), groups


def decompress_segments_device(d_comp, seg_offsets, n_words, first_segment=0, n_segments=None, out=None, workspace=None,
                               check=True):
    """Segments [first_segment, first_segment + n_segments) of the bitmap (992 words each, the last one shorter) from a
    stream of an `indexed` compressor and its seg_offsets, without scanning the stream (wah_decompress_segments_device).
    `out` / `workspace`: reuse these tensors; check=False: only enqueue (the caller reads the status later)."""
    torch = _torch()
    _as_words(torch, d_comp)
    groups = max_compressed_words(int(n_words))
    all_segments = (groups + 1023) // 1024
    if n_segments is None:
        n_segments = all_segments - first_segment
    total = decoded_words(groups)
    need = max(0, min((first_segment + n_segments) * 992, total) - first_segment * 992) if n_segments else 0
    if out is None:
        out = torch.empty(max(need, 1), dtype=torch.int32, device=d_comp.device)
    ws_bytes = int(lib().wah_decompress_segments_workspace_bytes())
    if workspace is None:
        workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=d_comp.device)
    rc = lib().wah_decompress_segments_device(d_comp.data_ptr(), d_comp.numel(), seg_offsets.data_ptr(), int(n_words),
                                              int(first_segment), int(n_segments), out.data_ptr(), out.numel(),
                                              workspace.data_ptr(), workspace.numel(), _stream_ptr(torch))
    _check(rc, "wah_decompress_segments_device")
    if check:
        _check(lib().wah_decompress_status(workspace.data_ptr(), _stream_ptr(torch)), "decompress_segments")
    return out[:need]


def merge_fills_device(d_comp):
    """The stream with adjacent fills of one kind merged and empty fills dropped: unsegmented WAH (wah_merge_fills_device)."""
    torch = _torch()
    _as_words(torch, d_comp)
    c = int(d_comp.numel())
    ws_bytes = int(lib().wah_merge_fills_workspace_bytes(c))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=d_comp.device)
    out = torch.empty(max(c, 1), dtype=torch.int32, device=d_comp.device)
    count = torch.zeros(1, dtype=torch.int64, device=d_comp.device)
    sp = _stream_ptr(torch)
    _check(lib().wah_merge_fills_device(d_comp.data_ptr(), c, out.data_ptr(), c, count.data_ptr(), ws.data_ptr(), ws_bytes, sp),
           "wah_merge_fills_device")
    _check(lib().wah_decompress_status(ws.data_ptr(), sp), "merge_fills")
    return out[: int(count.item())].clone()


OPS = {"and": 0, "or": 1, "xor": 2, "andnot": 3}


def bitop_device(op, d_a, d_b, n_words):
    """compress(A op B) from the two compressed bitmaps of n_words words each (include/wah.h: wah_bitop_device)."""
    torch = _torch()
    _as_words(torch, d_a)
    _as_words(torch, d_b)
    n, ca, cb = int(n_words), int(d_a.numel()), int(d_b.numel())
    cap = max_compressed_words(n)
    sc_bytes = int(lib().wah_bitop_scratch_bytes(n, ca, cb))
    scratch = torch.empty(sc_bytes, dtype=torch.uint8, device=d_a.device)
    out = torch.empty(max(cap, 1), dtype=torch.int32, device=d_a.device)
    count = torch.zeros(1, dtype=torch.int64, device=d_a.device)
    sp = _stream_ptr(torch)
    _check(lib().wah_bitop_device(OPS[op], n, d_a.data_ptr(), ca, d_b.data_ptr(), cb, out.data_ptr(), cap, count.data_ptr(),
                                  scratch.data_ptr(), sc_bytes, sp), "wah_bitop_device")
    _check(lib().wah_bitop_status(scratch.data_ptr(), n, ca, cb, sp), "bitop")
    return out[: int(count.item())].clone()


def _as_int64(v, what):
    """A Python int in 0 .. 2^64 - 1 as the int64 of the same bit pattern; what: how the refusal names the number."""
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise WahError(f"{what} is an unsigned integer below 2^64")
    return v - (1 << 64) if v >= 1 << 63 else v


def _int64_tensor(torch, given, shape, dev, refusal):
    """The int64 tensor a call writes a result into: `given` when it is contiguous, of this shape and on dev, a new one when the
    caller passed None; anything else raises WahError(refusal)."""
    if given is None:
        return torch.empty(shape, dtype=torch.int64, device=dev)
    if given.dtype != torch.int64 or tuple(given.shape) != tuple(shape) or given.device != dev or not given.is_contiguous():
        raise WahError(refusal)
    return given


def _enqueued(name, what, enqueue, status, scratch, check):
    """The tail of the calls that leave their results in tensors of the caller's: enqueue(*tail), the C call `name` with its
    leading arguments bound -- tail is what all of them end with, (scratch, its bytes, stream) -- and, unless check=False,
    status(scratch pointer, stream) read under the name `what`."""
    sp = _stream_ptr(_torch())
    _check(enqueue(scratch.data_ptr(), scratch.numel(), sp), name)
    if check:
        _check(status(scratch.data_ptr(), sp), what)


def _compressed(name, what, dev, enqueue, status, scratch, out, out_offsets, entries, check):
    """The tail of the calls that return compressed words with their segment index: enqueue(*tail), the C call `name` with its
    leading arguments bound -- tail is what all of them end with, (out, its capacity, count, out_offsets, scratch, its bytes,
    stream).  check=False: returns (out, count tensor, out_offsets); otherwise status(scratch pointer, stream) is read under the
    name `what` and the result is (out[:count], out_offsets[:entries]), the index as it is when entries is None."""
    torch = _torch()
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    sp = _stream_ptr(torch)
    _check(enqueue(out.data_ptr(), out.numel(), count.data_ptr(), out_offsets.data_ptr(), scratch.data_ptr(), scratch.numel(), sp), name)
    if not check:
        return out, count, out_offsets
    _check(status(scratch.data_ptr(), sp), what)
    return out[: int(count.item())], out_offsets if entries is None else out_offsets[:entries]


def _compressed_result(name, n_words, dev, scratch_bytes, enqueue, status, scratch, out, out_offsets, check):
    """What the calls that return ONE compressed bitmap with its segment index share.  Allocates what the caller did not pass --
    scratch of scratch_bytes() bytes, out of max_compressed_words words, out_offsets of one entry per segment + 1 -- and goes on
    as _compressed, the index returned whole."""
    torch = _torch()
    cap = max_compressed_words(n_words)
    if scratch is None:
        scratch = torch.empty(int(scratch_bytes()), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
    if out_offsets is None:
        out_offsets = torch.zeros((cap + 1023) // 1024 + 1, dtype=torch.int64, device=dev)
    return _compressed(name, name[len("wah_"):-len("_device")], dev, enqueue, status, scratch, out, out_offsets, None, check)


def _compressed_streams(name, what, dev, entries, offsets_refusal, scratch_bytes, out_words, enqueue, status, scratch, out, out_offsets, check):
    """What the calls that return SEVERAL streams back to back with one index of `entries` entries share.  Allocates what the caller
    did not pass -- scratch of scratch_bytes() bytes, out of out_words() words, out_offsets of `entries` -- judges what it did pass
    (out_offsets too short or of another kind: WahError(offsets_refusal)), and goes on as _compressed, the index cut to `entries`."""
    torch = _torch()
    if scratch is None:
        scratch = torch.empty(int(scratch_bytes()), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(out_words(), dtype=torch.int32, device=dev)
    else:
        _as_words(torch, out)
    if out_offsets is None:
        out_offsets = torch.empty(entries, dtype=torch.int64, device=dev)
    elif out_offsets.dtype != torch.int64 or out_offsets.numel() < entries or not out_offsets.is_contiguous() or out_offsets.device != dev:
        raise WahError(offsets_refusal)
    return _compressed(name, what, dev, enqueue, status, scratch, out, out_offsets, entries, check)


def bitop_indexed_device(op, d_a, a_offsets, d_b, b_offsets, n_words, scratch=None, out=None, out_offsets=None, check=True):
    """compress(A op B) from two compressed bitmaps that come with their segment indexes (wah_bitop_indexed_device).
    Returns (stream, seg_offsets) of the result; scratch / out / out_offsets: reuse these tensors; check=False: only
    enqueue and return (out, count tensor, out_offsets)."""
    torch = _torch()
    _as_words(torch, d_a)
    _as_words(torch, d_b)
    n = int(n_words)
    return _compressed_result(
        "wah_bitop_indexed_device", n, d_a.device, lambda: lib().wah_bitop_indexed_scratch_bytes(n),
        lambda *tail: lib().wah_bitop_indexed_device(OPS[op], n, d_a.data_ptr(), d_a.numel(), a_offsets.data_ptr(), d_b.data_ptr(),
                                                     d_b.numel(), b_offsets.data_ptr(), *tail),
        lambda sc, sp: lib().wah_bitop_indexed_status(sc, n, sp), scratch, out, out_offsets, check)


def bitop_many_indexed_device(op, operands, n_words, scratch=None, out=None, out_offsets=None, check=True):
    """compress(A op B op C ...) for up to 8 (stream, seg_offsets) pairs in one combining pass
    (wah_bitop_many_indexed_device).  Returns as bitop_indexed_device."""
    torch = _torch()
    k = len(operands)
    for st, _ in operands:
        _as_words(torch, st)
    n = int(n_words)
    streams = (ctypes.c_void_p * k)(*[st.data_ptr() for st, _ in operands])
    words = (ctypes.c_uint64 * k)(*[st.numel() for st, _ in operands])
    offsets = (ctypes.c_void_p * k)(*[o.data_ptr() for _, o in operands])
    return _compressed_result(
        "wah_bitop_many_indexed_device", n, operands[0][0].device, lambda: lib().wah_bitop_indexed_scratch_bytes(n),
        lambda *tail: lib().wah_bitop_many_indexed_device(OPS[op], n, k, streams, words, offsets, *tail),
        lambda sc, sp: lib().wah_bitop_indexed_status(sc, n, sp), scratch, out, out_offsets, check)


class BitopOperand(ctypes.Structure):
    """wah_bitop_operand of include/wah.h: one row of an operand table (24 bytes, no padding)."""
    _fields_ = [("d_stream", ctypes.c_void_p), ("stream_words", ctypes.c_uint64), ("d_offsets", ctypes.c_void_p)]


def bitop_operand_table(operands, device=None):
    """The wah_bitop_operand array of a list of (stream, seg_offsets) pairs of any length, as an int64 device tensor of
    shape [k, 3]: rows of (stream pointer, stream words, index pointer).  The table holds RAW POINTERS and no reference to
    the tensors they point into: the caller keeps those alive for as long as the table is used."""
    torch = _torch()
    if not operands:
        raise WahError("an operand table needs at least one operand")
    rows = []
    for st, offs in operands:
        _as_words(torch, st)
        if offs.dtype != torch.int64 or not offs.is_cuda or not offs.is_contiguous():
            raise WahError("a segment index is a contiguous int64 CUDA tensor")
        rows.append((st.data_ptr(), st.numel(), offs.data_ptr()))
    return torch.tensor(rows, dtype=torch.int64, device=operands[0][0].device if device is None else device)


def _operand_table(x, what="an operand table"):
    """x as the [k, 3] table the device reads: a list of (stream, seg_offsets) pairs is converted (bitop_operand_table), a
    ready tensor is checked."""
    torch = _torch()
    table = x if isinstance(x, torch.Tensor) else bitop_operand_table(x)
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or not table.is_cuda or not table.is_contiguous():
        raise WahError(f"{what} is a contiguous int64 CUDA tensor of shape [k, 3], k >= 1")
    return table


def bitop_list_indexed_device(op, operands, n_words, scratch=None, out=None, out_offsets=None, check=True):
    """compress(A op B op C ...) for ANY number of operands in one call (wah_bitop_list_indexed_device).  operands: a list of
    (stream, seg_offsets) pairs, or a ready table (bitop_operand_table, columns.column_operand_table) -- only the device
    reads it.  Returns as bitop_indexed_device: (stream, seg_offsets), or with check=False, which only enqueues,
    (out, count tensor, out_offsets)."""
    table = _operand_table(operands)
    n, k = int(n_words), int(table.shape[0])
    return _compressed_result(
        "wah_bitop_list_indexed_device", n, table.device, lambda: lib().wah_bitop_list_scratch_bytes(n, k),
        lambda *tail: lib().wah_bitop_list_indexed_device(OPS[op], n, k, table.data_ptr(), *tail),
        lambda sc, sp: lib().wah_bitop_list_status(sc, n, k, sp), scratch, out, out_offsets, check)


CLAUSE_NEGATE = -(1 << 63)  # WAH_CLAUSE_NEGATE (bit 63) as the int64 a clause table holds


def bitop_clause_table(clauses, device=None):
    """The two device tables of a conjunction of clauses (wah_bitop_clauses_indexed_device): clauses is a list of
    (operands, negate) with operands a non-empty list of (stream, seg_offsets) pairs.  Returns (operand_table [k, 3] int64,
    clause_ends [c] int64): the operands of all clauses back to back (bitop_operand_table), and per clause the index one past
    its last operand, bit 63 set for a negated clause.  The tables hold RAW POINTERS and no reference to the tensors they
    point into: the caller keeps those alive for as long as the tables are used."""
    torch = _torch()
    if not clauses:
        raise WahError("a clause table needs at least one clause")
    flat, ends = [], []
    for operands, negate in clauses:
        if not operands:
            raise WahError("a clause needs at least one operand")
        flat.extend(operands)
        ends.append(len(flat) | (CLAUSE_NEGATE if negate else 0))
    table = bitop_operand_table(flat, device=device)
    return table, torch.tensor(ends, dtype=torch.int64, device=table.device)


def bitop_clauses_indexed_device(clauses, n_words, scratch=None, out=None, out_offsets=None, check=True):
    """compress(AND over clauses of [NOT] (OR of the clause's operands)) in one call (wah_bitop_clauses_indexed_device): a
    conjunction of IN / NOT IN lists over a bitmap index.  clauses: a list of (operands, negate) as for bitop_clause_table,
    or the ready pair (operand_table, clause_ends) -- only the device reads them.  Returns as bitop_list_indexed_device:
    (stream, seg_offsets), or with check=False, which only enqueues, (out, count tensor, out_offsets)."""
    torch = _torch()
    ready = isinstance(clauses, (tuple, list)) and len(clauses) == 2 and all(isinstance(t, torch.Tensor) for t in clauses)
    table, ends = clauses if ready else bitop_clause_table(clauses)
    table = _operand_table(table)
    if ends.dtype != torch.int64 or ends.dim() != 1 or not 1 <= ends.shape[0] <= table.shape[0] or ends.device != table.device or not ends.is_contiguous():
        raise WahError("clause ends are a contiguous int64 tensor of 1 to k entries on the operand table's device")
    n, k, c = int(n_words), int(table.shape[0]), int(ends.shape[0])
    return _compressed_result(
        "wah_bitop_clauses_indexed_device", n, table.device, lambda: lib().wah_bitop_clauses_scratch_bytes(n, k, c),
        lambda *tail: lib().wah_bitop_clauses_indexed_device(n, c, ends.data_ptr(), k, table.data_ptr(), *tail),
        lambda sc, sp: lib().wah_bitop_clauses_status(sc, n, k, c, sp), scratch, out, out_offsets, check)


BSI_MAX_SLICES = 64  # WAH_BSI_MAX_SLICES
BSI_EXISTS = 1  # WAH_BSI_EXISTS


def bsi_bounds(lo, hi, device, out=None):
    """The bounds of wah_bsi_range_indexed_device as an int64 device tensor [2]: two Python ints in 0 .. 2^64 - 1, stored as
    their two's-complement bit patterns.  out: an existing tensor to overwrite in place -- what a captured graph replayed
    with another range needs."""
    import torch

    t = torch.tensor([_as_int64(v, "a bound") for v in (lo, hi)], dtype=torch.int64)
    if out is None:
        return t.to(device)
    out.copy_(t)
    return out


def bsi_range_device(table, bounds, n_words, exists=False, scratch=None, out=None, out_offsets=None, check=True):
    """compress(lo <= value <= hi [AND exists]) over a bit-sliced attribute in one call (wah_bsi_range_indexed_device).  table:
    a list of (stream, seg_offsets) pairs or a ready [rows, 3] table (bitop_operand_table, columns.column_operand_table), one
    row per slice, MOST significant first, and with exists=True the existence bitmap as one more row behind them.  bounds: an
    int64 device tensor [2] (lo, hi as 64-bit patterns; only the device reads it) or a (lo, hi) pair of Python ints up to
    2^64 - 1 (bsi_bounds).  Returns as bitop_clauses_indexed_device: (stream, seg_offsets), or with check=False, which only
    enqueues, (out, count tensor, out_offsets)."""
    torch = _torch()
    table = _operand_table(table, "a slice table")
    dev = table.device
    k = int(table.shape[0]) - (1 if exists else 0)
    if not 1 <= k <= BSI_MAX_SLICES:
        raise WahError("between 1 and 64 slices (and one more row with exists=True)")
    if not isinstance(bounds, torch.Tensor):
        lo, hi = bounds
        bounds = bsi_bounds(lo, hi, dev)
    if bounds.dtype != torch.int64 or tuple(bounds.shape) != (2,) or bounds.device != dev or not bounds.is_contiguous():
        raise WahError("bounds: a contiguous int64 [2] tensor on the table's device, or a (lo, hi) pair")
    n = int(n_words)
    return _compressed_result(
        "wah_bsi_range_indexed_device", n, dev, lambda: lib().wah_bsi_range_scratch_bytes(n, k),
        lambda *tail: lib().wah_bsi_range_indexed_device(n, k, table.data_ptr(), bounds.data_ptr(), BSI_EXISTS if exists else 0, *tail),
        lambda sc, sp: lib().wah_bsi_range_status(sc, n, k, sp), scratch, out, out_offsets, check)


MEMBER_NEGATE, MEMBER_BITSET = 2, 4  # WAH_MEMBER_NEGATE, WAH_MEMBER_BITSET


def member_set(values, device):
    """The set of wah_bsi_member_indexed_device as the sorted int64 device tensor the call reads: values are Python ints in
    0 .. 2^64 - 1 or a numpy uint64 array, sorted as UNSIGNED numbers and stored as their two's-complement bit patterns, the way
    bsi_bounds stores a bound.  Duplicates stay: the call allows them."""
    import torch

    if isinstance(values, np.ndarray):
        if values.dtype != np.uint64:
            raise WahError("a numpy set is a uint64 array")
        v = np.sort(values.reshape(-1))
    else:
        v = np.array(sorted(_as_int64(x, "a set entry") & ((1 << 64) - 1) for x in values), dtype=np.uint64)
    return torch.from_numpy(v.view(np.int64).copy()).to(device)


def bsi_member_device(table, members, n_words, count=None, exists=False, negate=False, bitset=False, set_bits=None, scratch=None, out=None,
                      out_offsets=None, check=True):
    """compress(value IN members [AND exists]) -- negate=True: NOT IN -- over a bit-sliced attribute in one call
    (wah_bsi_member_indexed_device).  table: as for bsi_range_device, one row per slice, MOST significant first, and with
    exists=True the existence bitmap as one more row behind them.  members: a contiguous int64 device tensor, the set as 64-bit
    patterns in non-decreasing UNSIGNED order (member_set; duplicates allowed), of which the first count[0] entries count when
    count, an int64 device tensor [1], is given -- or with bitset=True a contiguous int32 device tensor of words, a bit array of
    set_bits bits (default: 32 per word) in which value v is bit v % 32 of word v / 32: a decoded bitmap.  Only the device reads
    members and count.  Returns as bsi_range_device: (stream, seg_offsets), or with check=False, which only enqueues, (out, count
    tensor, out_offsets)."""
    torch = _torch()
    table = _operand_table(table, "a slice table")
    dev = table.device
    k = int(table.shape[0]) - (1 if exists else 0)
    if not 1 <= k <= BSI_MAX_SLICES:
        raise WahError("between 1 and 64 slices (and one more row with exists=True)")
    if not isinstance(members, torch.Tensor) or members.dim() != 1 or members.device != dev or not members.is_contiguous():
        raise WahError("members: a contiguous one-dimensional tensor on the table's device")
    if bitset:
        if members.dtype not in (torch.int32, torch.uint32) or count is not None:
            raise WahError("a bit array is a 32-bit integer tensor of words and has no count")
        capacity = 32 * int(members.numel()) if set_bits is None else int(set_bits)
        if not 0 <= capacity <= 32 * int(members.numel()):
            raise WahError("set_bits: at most 32 bits per word of the bit array")
    else:
        if members.dtype != torch.int64 or set_bits is not None:
            raise WahError("a list is an int64 tensor (member_set) and has no set_bits")
        capacity = int(members.numel())
        if count is not None and (count.dtype != torch.int64 or count.numel() != 1 or count.device != dev):
            raise WahError("count: a one-element int64 tensor on the table's device")
    flags = (BSI_EXISTS if exists else 0) | (MEMBER_NEGATE if negate else 0) | (MEMBER_BITSET if bitset else 0)
    set_ptr = members.data_ptr() if members.numel() else None
    count_ptr = None if count is None else count.data_ptr()
    n = int(n_words)
    return _compressed_result(
        "wah_bsi_member_indexed_device", n, dev, lambda: lib().wah_bsi_member_scratch_bytes(n, k),
        lambda *tail: lib().wah_bsi_member_indexed_device(n, k, table.data_ptr(), set_ptr, capacity, count_ptr, flags, *tail),
        lambda sc, sp: lib().wah_bsi_member_status(sc, n, k, sp), scratch, out, out_offsets, check)


BSI_EXISTS_A, BSI_EXISTS_B = 1, 2  # WAH_BSI_EXISTS_A, WAH_BSI_EXISTS_B
CMP_OPS = {"<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5}  # WAH_CMP_*


def bsi_compare_row_order(ka, kb, exists_a=False, exists_b=False):
    """The table order of wah_bsi_compare_indexed_device for attributes of ka and kb slices, as a list of (attribute, slice
    index) with attribute "a" or "b" and the slice index counted as in an attribute's own table: 0 is its MOST significant
    slice, ka (kb) its existence bitmap.  The slices are interleaved by significance, most significant first, A's before B's
    where both have one; then A's existence row, then B's.  Needs neither torch nor a device."""
    ka, kb = int(ka), int(kb)
    if not (1 <= ka <= BSI_MAX_SLICES and 1 <= kb <= BSI_MAX_SLICES):
        raise WahError("between 1 and 64 slices per attribute")
    order = []
    for sig in range(max(ka, kb) - 1, -1, -1):
        if sig < ka:
            order.append(("a", ka - 1 - sig))
        if sig < kb:
            order.append(("b", kb - 1 - sig))
    if exists_a:
        order.append(("a", ka))
    if exists_b:
        order.append(("b", kb))
    return order


def bsi_compare_device(table, n_bits_a, n_bits_b, op, n_words, exists_a=False, exists_b=False, scratch=None, out=None, out_offsets=None,
                       check=True):
    """compress(A op B [AND exists]) row by row over two bit-sliced attributes in one call (wah_bsi_compare_indexed_device).
    table: a list of (stream, seg_offsets) pairs or a ready [rows, 3] table in the order of bsi_compare_row_order(n_bits_a,
    n_bits_b, exists_a, exists_b) -- only the device reads it.  op: a key of CMP_OPS; both values are read as unsigned.
    Returns as bsi_range_device: (stream, seg_offsets), or with check=False, which only enqueues, (out, count tensor,
    out_offsets)."""
    if op not in CMP_OPS:
        raise WahError(f"a comparison is one of {', '.join(CMP_OPS)}")
    table = _operand_table(table, "a row table")
    ka, kb = int(n_bits_a), int(n_bits_b)
    flags = (BSI_EXISTS_A if exists_a else 0) | (BSI_EXISTS_B if exists_b else 0)
    if not (1 <= ka <= BSI_MAX_SLICES and 1 <= kb <= BSI_MAX_SLICES):
        raise WahError("between 1 and 64 slices per attribute")
    if int(table.shape[0]) != ka + kb + bool(exists_a) + bool(exists_b):
        raise WahError("the table has one row per slice of either attribute and one per existence bitmap")
    n, code = int(n_words), CMP_OPS[op]
    return _compressed_result(
        "wah_bsi_compare_indexed_device", n, table.device, lambda: lib().wah_bsi_compare_scratch_bytes(n, ka, kb),
        lambda *tail: lib().wah_bsi_compare_indexed_device(code, n, ka, kb, table.data_ptr(), flags, *tail),
        lambda sc, sp: lib().wah_bsi_compare_status(sc, n, ka, kb, sp), scratch, out, out_offsets, check)


ARITH_OPS = {"+": 0, "-": 1}  # WAH_ARITH_*


def bsi_arith_row_order(ka, kb, exists_a=False, exists_b=False):
    """The table order of wah_bsi_arith_indexed_device for attributes of ka and kb slices, as a list of (attribute, slice index)
    counted as in bsi_compare_row_order: 0 is an attribute's MOST significant slice, ka (kb) its existence bitmap.  A's existence
    row, then B's, come FIRST; then the slices interleaved by significance, LEAST significant first, A's before B's where both
    have one -- the carry runs upwards.  Needs neither torch nor a device."""
    ka, kb = int(ka), int(kb)
    if not (1 <= ka <= BSI_MAX_SLICES and 1 <= kb <= BSI_MAX_SLICES):
        raise WahError("between 1 and 64 slices per attribute")
    order = []
    if exists_a:
        order.append(("a", ka))
    if exists_b:
        order.append(("b", kb))
    for sig in range(max(ka, kb)):
        if sig < ka:
            order.append(("a", ka - 1 - sig))
        if sig < kb:
            order.append(("b", kb - 1 - sig))
    return order


_ROWS_OUT_OFFSETS = "out_offsets: a contiguous int64 tensor of rows_out * n_words / 992 + 1 entries on the table's device"


def _two_attributes(table, n_bits_a, n_bits_b, n_bits_out, n_words, exists_a, exists_b):
    """The arguments of the calls that compute a new attribute from two (bsi_arith_device, bsi_mul_device), judged: the checked
    table, the three widths and n_words as ints, the existence flags, and the result's rows (its slices, and an existence bitmap
    where an operand has one)."""
    table = _operand_table(table, "a row table")
    ka, kb, k_out, n = int(n_bits_a), int(n_bits_b), int(n_bits_out), int(n_words)
    flags = (BSI_EXISTS_A if exists_a else 0) | (BSI_EXISTS_B if exists_b else 0)
    if not (1 <= ka <= BSI_MAX_SLICES and 1 <= kb <= BSI_MAX_SLICES and 1 <= k_out <= BSI_MAX_SLICES):
        raise WahError("between 1 and 64 slices per attribute and in the result")
    if int(table.shape[0]) != ka + kb + bool(exists_a) + bool(exists_b):
        raise WahError("the table has one row per slice of either attribute and one per existence bitmap")
    if n <= 0 or n % 992:
        raise WahError("slices of a multiple of 992 words")
    return table, ka, kb, k_out, n, flags, k_out + (1 if flags else 0)


def bsi_arith_device(table, n_bits_a, n_bits_b, op, n_bits_out, n_words, exists_a=False, exists_b=False, scratch=None, out=None,
                     out_offsets=None, check=True):
    """The bit-sliced index of (A op B) mod 2^n_bits_out, row by row over two bit-sliced attributes, in one call
    (wah_bsi_arith_indexed_device).  table: a list of (stream, seg_offsets) pairs or a ready [rows, 3] table in the order of
    bsi_arith_row_order(n_bits_a, n_bits_b, exists_a, exists_b) -- only the device reads it.  op: a key of ARITH_OPS; both values
    are read as unsigned.  n_bits_out: 1 .. 64; max(n_bits_a, n_bits_b) + 1 never loses a carry, and for "-" that top slice is set
    exactly where A < B.  n_words: the words of one slice, a multiple of 992.  With an existence flag the result has an existence
    bitmap, the AND of those present, as its last slice.  Returns as bsi_build_device: (stream, seg_offsets), the slices'
    compress() streams back to back, MOST significant first, and the rows_out * (n_words / 992) + 1 entries of their segment
    index; scratch / out / out_offsets: reuse these tensors; check=False: only enqueue and return (out, count tensor, out_offsets)
    -- the caller reads wah_bsi_arith_status later."""
    if op not in ARITH_OPS:
        raise WahError(f"an arithmetic operation is one of {', '.join(ARITH_OPS)}")
    table, ka, kb, k_out, n, flags, rows_out = _two_attributes(table, n_bits_a, n_bits_b, n_bits_out, n_words, exists_a, exists_b)
    return _compressed_streams(
        "wah_bsi_arith_indexed_device", "bsi_arith", table.device, rows_out * (n // 992) + 1, _ROWS_OUT_OFFSETS,
        lambda: lib().wah_bsi_arith_scratch_bytes(n, k_out, flags), lambda: max_compressed_words(rows_out * n),
        lambda *tail: lib().wah_bsi_arith_indexed_device(ARITH_OPS[op], n, ka, kb, k_out, table.data_ptr(), flags, *tail),
        lambda sc, sp: lib().wah_bsi_arith_status(sc, n, k_out, flags, sp), scratch, out, out_offsets, check)


def bsi_mul_row_order(ka, kb, exists_a=False, exists_b=False):
    """The table order of wah_bsi_mul_indexed_device for attributes of ka and kb slices, as a list of (attribute, slice index)
    counted as in bsi_compare_row_order: 0 is an attribute's MOST significant slice, ka (kb) its existence bitmap.  A's existence
    row, then B's, come FIRST; then ALL of A's slices, LEAST significant first; then ALL of B's, LEAST significant first -- no
    interleaving: every slice of B meets the whole of A.  Needs neither torch nor a device."""
    ka, kb = int(ka), int(kb)
    if not (1 <= ka <= BSI_MAX_SLICES and 1 <= kb <= BSI_MAX_SLICES):
        raise WahError("between 1 and 64 slices per attribute")
    order = []
    if exists_a:
        order.append(("a", ka))
    if exists_b:
        order.append(("b", kb))
    order += [("a", ka - 1 - sig) for sig in range(ka)]
    order += [("b", kb - 1 - sig) for sig in range(kb)]
    return order


def bsi_mul_device(table, n_bits_a, n_bits_b, n_bits_out, n_words, exists_a=False, exists_b=False, scratch=None, out=None,
                   out_offsets=None, check=True):
    """The bit-sliced index of (A * B) mod 2^n_bits_out, row by row over two bit-sliced attributes, in one call
    (wah_bsi_mul_indexed_device).  table: a list of (stream, seg_offsets) pairs or a ready [rows, 3] table in the order of
    bsi_mul_row_order(n_bits_a, n_bits_b, exists_a, exists_b) -- only the device reads it.  Both values are read as unsigned.
    n_bits_out: 1 .. 64; n_bits_a + n_bits_b loses nothing, fewer truncate, more zero-extend.  The call takes the operands as
    given; the narrower one as A keeps the scratch small.  n_words, the existence flags, the result and scratch / out /
    out_offsets / check: as bsi_arith_device -- with check=False the caller reads wah_bsi_mul_status later."""
    table, ka, kb, k_out, n, flags, rows_out = _two_attributes(table, n_bits_a, n_bits_b, n_bits_out, n_words, exists_a, exists_b)
    return _compressed_streams(
        "wah_bsi_mul_indexed_device", "bsi_mul", table.device, rows_out * (n // 992) + 1, _ROWS_OUT_OFFSETS,
        lambda: lib().wah_bsi_mul_scratch_bytes(n, ka, k_out, flags), lambda: max_compressed_words(rows_out * n),
        lambda *tail: lib().wah_bsi_mul_indexed_device(n, ka, kb, k_out, table.data_ptr(), flags, *tail),
        lambda sc, sp: lib().wah_bsi_mul_status(sc, n, ka, k_out, flags, sp), scratch, out, out_offsets, check)


DIV_QUOTIENT, DIV_REMAINDER = 0, 1  # WAH_DIV_*


def bsi_div_row_order(ka, kb, exists_a=False, exists_b=False):
    """The table order of wah_bsi_div_indexed_device for a dividend A of ka and a divisor B of kb slices, as a list of (attribute,
    slice index) counted as in bsi_compare_row_order: 0 is an attribute's MOST significant slice, ka (kb) its existence bitmap.
    A's existence row, then B's, come FIRST; then ALL of B's slices, LEAST significant first; then ALL of A's, MOST significant
    first -- the divisor is whole before long division takes the dividend from the top.  Needs neither torch nor a device."""
    ka, kb = int(ka), int(kb)
    if not (1 <= ka <= BSI_MAX_SLICES and 1 <= kb <= BSI_MAX_SLICES):
        raise WahError("between 1 and 64 slices per attribute")
    order = []
    if exists_a:
        order.append(("a", ka))
    if exists_b:
        order.append(("b", kb))
    order += [("b", kb - 1 - sig) for sig in range(kb)]
    order += [("a", i) for i in range(ka)]
    return order


def bsi_div_device(table, n_bits_a, n_bits_b, n_bits_out, n_words, remainder=False, exists_a=False, exists_b=False, scratch=None,
                   out=None, out_offsets=None, check=True):
    """The bit-sliced index of floor(A / B) mod 2^n_bits_out -- with remainder=True of (A mod B) mod 2^n_bits_out -- row by row
    over two bit-sliced attributes, in one call (wah_bsi_div_indexed_device).  table: a list of (stream, seg_offsets) pairs or a
    ready [rows, 3] table in the order of bsi_div_row_order(n_bits_a, n_bits_b, exists_a, exists_b) -- only the device reads it.
    Both values are read as unsigned.  n_bits_out: 1 .. 64; n_bits_a loses nothing of the quotient, min(n_bits_a, n_bits_b)
    nothing of the remainder, fewer truncate, more zero-extend.  The result ALWAYS has an existence bitmap as its last slice:
    the AND of the operands' bitmaps that are there and of B != 0 -- a division by zero is NULL.  n_words, the result and
    scratch / out / out_offsets / check: as bsi_mul_device with n_bits_out + 1 rows -- with check=False the caller reads
    wah_bsi_div_status later."""
    table, ka, kb, k_out, n, flags, _ = _two_attributes(table, n_bits_a, n_bits_b, n_bits_out, n_words, exists_a, exists_b)
    what, rows_out = (DIV_REMAINDER if remainder else DIV_QUOTIENT), k_out + 1
    return _compressed_streams(
        "wah_bsi_div_indexed_device", "bsi_div", table.device, rows_out * (n // 992) + 1, _ROWS_OUT_OFFSETS,
        lambda: lib().wah_bsi_div_scratch_bytes(n, kb, k_out, flags), lambda: max_compressed_words(rows_out * n),
        lambda *tail: lib().wah_bsi_div_indexed_device(what, n, ka, kb, k_out, table.data_ptr(), flags, *tail),
        lambda sc, sp: lib().wah_bsi_div_status(sc, n, kb, k_out, flags, sp), scratch, out, out_offsets, check)


BSI_KTH_ASCENDING, BSI_KTH_DESCENDING, BSI_KTH_QUANTILE = 0, 1, 2  # WAH_BSI_KTH_*
BSI_KTH_MAX_FILTERS = 64  # WAH_BSI_KTH_MAX_FILTERS


def bsi_kth_query(kind, a, b=1, device="cuda:0", out=None):
    """The query of wah_bsi_kth_indexed_device as an int64 device tensor [3]: {kind, a, b}, three Python ints in 0 .. 2^64 - 1
    stored as their two's-complement bit patterns.  BSI_KTH_ASCENDING / BSI_KTH_DESCENDING: rank a from the bottom / the top,
    0-based; BSI_KTH_QUANTILE: rank floor(a * (total - 1) / b) from the bottom.  Nothing is judged here: an unknown kind, b == 0
    or a > b are answered by the device with found = 0.  out: an existing tensor to overwrite in place -- what a captured graph
    replayed with another query needs."""
    import torch

    t = torch.tensor([_as_int64(v, "a query word") for v in (kind, a, b)], dtype=torch.int64)
    if out is None:
        return t.to(device)
    out.copy_(t)
    return out


def bsi_kth_device(table, query, n_words, n_filters, scratch=None, result=None, check=True):
    """The value of a given rank among the rows the filters select, over a bit-sliced attribute, in one call
    (wah_bsi_kth_indexed_device).  table: a list of (stream, seg_offsets) pairs or a ready [rows, 3] table (bitop_operand_table,
    columns.column_operand_table): n_filters filter rows FIRST, then one row per slice, MOST significant first.  query: an int64
    device tensor [3] (bsi_kth_query; only the device reads it) or a (kind, a, b) triple of Python ints.  Returns the int64
    device tensor [5] {found, value, total, less, equal} (64-bit patterns: a value at or above 2^63 reads as negative).
    scratch / result: reuse these tensors; check=False: only enqueue (the caller reads wah_bsi_kth_status later)."""
    torch = _torch()
    table = _operand_table(table, "a row table")
    dev = table.device
    f = int(n_filters)
    k = int(table.shape[0]) - f
    if not 0 <= f <= BSI_KTH_MAX_FILTERS or not 1 <= k <= BSI_MAX_SLICES:
        raise WahError("at most 64 filter rows, then between 1 and 64 slices")
    if not isinstance(query, torch.Tensor):
        query = bsi_kth_query(*query, device=dev)
    if query.dtype != torch.int64 or tuple(query.shape) != (3,) or query.device != dev or not query.is_contiguous():
        raise WahError("query: a contiguous int64 [3] tensor on the table's device, or a (kind, a, b) triple")
    n = int(n_words)
    if scratch is None:
        scratch = torch.empty(int(lib().wah_bsi_kth_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
    result = _int64_tensor(torch, result, (5,), dev, "result: a contiguous int64 [5] tensor on the table's device")
    _enqueued("wah_bsi_kth_indexed_device", "bsi_kth",
              lambda *tail: lib().wah_bsi_kth_indexed_device(n, f, k, table.data_ptr(), query.data_ptr(), result.data_ptr(), *tail),
              lib().wah_bsi_kth_status, scratch, check)
    return result


BSI_KTH_GROUPED_MAX_LANES = 4096  # WAH_BSI_KTH_GROUPED_MAX_LANES


def bsi_kth_queries(queries, device="cuda:0", out=None):
    """The query list of wah_bsi_kth_grouped_indexed_device as an int64 device tensor [Q, 3]: the many-row form of bsi_kth_query, one
    (kind, a, b) of Python ints in 0 .. 2^64 - 1 per row, stored as their two's-complement bit patterns.  Nothing is judged here.
    out: an existing [Q, 3] tensor to overwrite in place -- what a captured graph replayed with other queries needs."""
    import torch

    rows = []
    for query in queries:
        kind, a, b = query
        rows.append([_as_int64(v, "a query word") for v in (kind, a, b)])
    if not rows:
        raise WahError("at least one query")
    t = torch.tensor(rows, dtype=torch.int64)
    if out is None:
        return t.to(device)
    if out.dtype != torch.int64 or tuple(out.shape) != tuple(t.shape):
        raise WahError("out: an int64 [Q, 3] tensor")
    out.copy_(t)
    return out


def bsi_kth_grouped_device(filters, groups, slices, queries, n_words, rows_per_group=1, scratch=None, results=None, check=True):
    """`SELECT g, MIN(x), MAX(x), median(x) WHERE <filters> GROUP BY g` over ONE bit-sliced attribute in one call, nothing read back
    and no bitmap written (wah_bsi_kth_grouped_indexed_device): for every group and every query the value of that rank among the
    rows that all `filters` rows (None or empty: no filter) AND rows g * rows_per_group .. of `groups` select.  The three tables as
    group_sum_device takes them: each a list of (stream, seg_offsets) pairs, or a ready [k, 3] table (bitop_operand_table,
    columns.column_operand_table) -- only the device reads them; `slices`: one row per slice, MOST significant first.  queries: an
    int64 device tensor [Q, 3] (bsi_kth_queries) or a list of (kind, a, b) triples; G * Q <= 4096.  Returns the int64 device tensor
    [G, Q, 5] of {found, value, total, less, equal} (64-bit patterns: a value at or above 2^63 reads as negative).  scratch /
    results: reuse these tensors; check=False: only enqueue (the caller reads wah_bsi_kth_grouped_status later)."""
    torch = _torch()
    gt, st = _operand_table(groups, "a group table"), _operand_table(slices, "a slice table")
    dev = st.device
    ft = _operand_table(filters, "a filter table") if filters is not None and len(filters) else None
    if gt.device != dev or (ft is not None and ft.device != dev):
        raise WahError("the filter table, the group table and the slice table are on one device")
    r = int(rows_per_group)
    if r < 1 or r > GROUP_MAX_ROWS or gt.shape[0] % r:
        raise WahError("the group table holds 1 .. 8 rows (rows_per_group) for every group")
    if not isinstance(queries, torch.Tensor):
        queries = bsi_kth_queries(queries, device=dev)
    if queries.dtype != torch.int64 or queries.dim() != 2 or queries.shape[1] != 3 or queries.shape[0] < 1 or queries.device != dev or not queries.is_contiguous():
        raise WahError("queries: a contiguous int64 [Q, 3] tensor, Q >= 1, on the tables' device, or a list of (kind, a, b) triples")
    n, f, g, k, q = int(n_words), 0 if ft is None else int(ft.shape[0]), int(gt.shape[0]) // r, int(st.shape[0]), int(queries.shape[0])
    if f > BSI_KTH_MAX_FILTERS or k > BSI_MAX_SLICES or g * q > BSI_KTH_GROUPED_MAX_LANES:
        raise WahError("at most 64 filter rows, 64 slices and 4096 (group, query) pairs")
    if scratch is None:
        scratch = torch.empty(int(lib().wah_bsi_kth_grouped_scratch_bytes(n, k, g, q)), dtype=torch.uint8, device=dev)
    results = _int64_tensor(torch, results, (g, q, 5), dev, "results: a contiguous int64 [G, Q, 5] tensor on the tables' device")
    _enqueued("wah_bsi_kth_grouped_indexed_device", "bsi_kth_grouped",
              lambda *tail: lib().wah_bsi_kth_grouped_indexed_device(n, f, ft.data_ptr() if f else None, g, r, gt.data_ptr(), k, st.data_ptr(), q,
                                                                     queries.data_ptr(), results.data_ptr(), *tail),
              lib().wah_bsi_kth_grouped_status, scratch, check)
    return results


FETCH_BITS, FETCH_FIRST = 0, 1  # WAH_FETCH_*


def fetch_device(table, rows, n_words, mode, scratch=None, out=None, check=True):
    """The values of listed rows in one call, without decoding a bitmap (wah_fetch_indexed_device).  table: a list of (stream,
    seg_offsets) pairs or a ready [k, 3] table (bitop_operand_table, columns.column_operand_table); rows: an int64 device tensor
    of positions, NON-DESCENDING, each below 32 * n_words -- only the device reads either.  mode FETCH_BITS: entry i of the
    result is the value whose bit k - 1 - j is bit rows[i] of table row j (row 0 most significant, k <= 64; 64-bit patterns: a
    value at or above 2^63 reads as negative); FETCH_FIRST: the lowest j whose bitmap has the bit set, -1 (UINT64_MAX) if none.
    Only the segments that hold a listed row are read and checked.  Returns the int64 device tensor [len(rows)].  scratch / out:
    reuse these tensors; check=False: only enqueue (the caller reads wah_fetch_status later)."""
    torch = _torch()
    table = _operand_table(table)
    dev = table.device
    if mode not in (FETCH_BITS, FETCH_FIRST):
        raise WahError("mode: FETCH_BITS or FETCH_FIRST")
    if rows.dtype != torch.int64 or rows.dim() != 1 or rows.device != dev or not rows.is_contiguous():
        raise WahError("rows: a contiguous one-dimensional int64 tensor on the table's device")
    n, k, r = int(n_words), int(table.shape[0]), int(rows.numel())
    if scratch is None:
        scratch = torch.empty(int(lib().wah_fetch_scratch_bytes(n, r)), dtype=torch.uint8, device=dev)
    out = _int64_tensor(torch, out, (r,), dev, "out: a contiguous int64 [len(rows)] tensor on the table's device")
    _enqueued("wah_fetch_indexed_device", "fetch",
              lambda *tail: lib().wah_fetch_indexed_device(mode, n, k, table.data_ptr(), rows.data_ptr() if r else None, r,
                                                           out.data_ptr() if r else None, *tail),
              lib().wah_fetch_status, scratch, check)
    return out


def values_device(table, n_words, mode, first_row=0, n_rows=None, scratch=None, out=None, check=True):
    """The values of the row range [first_row, first_row + n_rows) in one call, a whole attribute read back out of the index
    (wah_values_indexed_device).  table and mode as for fetch_device; first_row / n_rows: Python ints, the window, n_rows
    defaulting to the rows behind first_row (32 * n_words - first_row).  Entry i of the result is what fetch_device gives for the
    listed row first_row + i.  Only the segments that overlap the window are read and checked.  Returns the int64 device tensor
    [n_rows].  scratch / out: reuse these tensors; check=False: only enqueue (the caller reads wah_values_status later)."""
    torch = _torch()
    table = _operand_table(table)
    dev = table.device
    if mode not in (FETCH_BITS, FETCH_FIRST):
        raise WahError("mode: FETCH_BITS or FETCH_FIRST")
    n, k, first = int(n_words), int(table.shape[0]), int(first_row)
    r = 32 * n - first if n_rows is None else int(n_rows)
    if first < 0 or r < 0:
        raise WahError("a window of rows inside the bitmap")
    if scratch is None:
        scratch = torch.empty(int(lib().wah_values_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
    out = _int64_tensor(torch, out, (r,), dev, "out: a contiguous int64 [n_rows] tensor on the table's device")
    _enqueued("wah_values_indexed_device", "values",
              lambda *tail: lib().wah_values_indexed_device(mode, n, k, table.data_ptr(), first, r, out.data_ptr() if r else None, *tail),
              lib().wah_values_status, scratch, check)
    return out


def count_device(operands_or_table, n_words, scratch=None, counts=None, check=True):
    """The set bits of every operand, counted in the compressed domain in one call (wah_count_list_indexed_device): an int64
    tensor [k], entry i for operand i.  operands_or_table: a list of (stream, seg_offsets) pairs, or a ready [k, 3] table
    (bitop_operand_table, columns.column_operand_table) -- only the device reads it.  The pad bits behind the bitmap's last
    word are never counted.  scratch / counts: reuse these tensors; check=False: only enqueue (the caller reads
    wah_select_status later)."""
    torch = _torch()
    table = _operand_table(operands_or_table)
    dev = table.device
    n, k = int(n_words), int(table.shape[0])
    if scratch is None:
        scratch = torch.empty(int(lib().wah_select_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
    counts = _int64_tensor(torch, counts, (k,), dev, "counts: a contiguous int64 [k] tensor on the table's device")
    _enqueued("wah_count_list_indexed_device", "count",
              lambda *tail: lib().wah_count_list_indexed_device(n, k, table.data_ptr(), counts.data_ptr(), *tail),
              lib().wah_select_status, scratch, check)
    return counts


def count_masked_device(masks, operands, n_words, scratch=None, counts=None, check=True):
    """The set bits every mask shares with every operand, counted in one call without decoding an operand or writing a bitmap
    (wah_count_masked_indexed_device): an int64 tensor [m, k], entry [i, j] the popcount of mask i AND operand j -- the GROUP BY
    histogram under a WHERE filter, a cross-tab.  masks / operands: each a list of (stream, seg_offsets) pairs, or a ready
    [m, 3] / [k, 3] table (bitop_operand_table, columns.column_operand_table) -- only the device reads them; m * k <= 2^24.  The
    pad bits behind the bitmap's last word are never counted.  scratch / counts: reuse these tensors (scratch as for
    count_device); check=False: only enqueue (the caller reads wah_select_status later)."""
    torch = _torch()
    mt, ot = _operand_table(masks, "a mask table"), _operand_table(operands)
    dev = ot.device
    if mt.device != dev:
        raise WahError("the mask table and the operand table are on one device")
    n, m, k = int(n_words), int(mt.shape[0]), int(ot.shape[0])
    if scratch is None:
        scratch = torch.empty(int(lib().wah_select_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
    counts = _int64_tensor(torch, counts, (m, k), dev, "counts: a contiguous int64 [m, k] tensor on the tables' device")
    _enqueued("wah_count_masked_indexed_device", "count_masked",
              lambda *tail: lib().wah_count_masked_indexed_device(n, m, mt.data_ptr(), k, ot.data_ptr(), counts.data_ptr(), *tail),
              lib().wah_select_status, scratch, check)
    return counts


GROUP_MAX_FILTERS, GROUP_MAX_ROWS, GROUP_MAX_ATTRS = 64, 8, 64  # WAH_GROUP_MAX_*


def group_sum_device(filters, groups, operands, attr_bits, n_words, rows_per_group=1, scratch=None, group_rows=None, counts=None,
                     sums=None, check=True):
    """`SELECT g, COUNT(*), SUM(x), SUM(y) WHERE <filters> GROUP BY g` over bit-sliced attributes in one call, no bitmap written
    and nothing read back (wah_group_sum_indexed_device).  The mask of group g is the AND of all `filters` rows (None or empty:
    no filter) and of rows g * rows_per_group .. of `groups` (1 .. 8 rows per group: one per grouping attribute); `operands` are
    the attributes' slices back to back, attribute t's attr_bits[t] slices most significant first (a host list of widths 1 .. 64
    that add up to the operand count; at most 64 attributes).  The three tables: each a list of (stream, seg_offsets) pairs, or a
    ready [k, 3] table (bitop_operand_table, columns.column_operand_table) -- only the device reads them; G * K <= 2^24.  Returns
    (group_rows [G], counts [G, K], sums [G, A, 2]) as int64 device tensors: COUNT(*) per group, the set bits every group's
    conjunction shares with every operand, and per attribute the low and high 64 bits of its sum (bit patterns: a low word at or
    above 2^63 reads as negative).  The pad bits behind the bitmap's last word are never counted.  scratch / group_rows / counts
    / sums: reuse these tensors (scratch as for count_device); check=False: only enqueue (the caller reads wah_select_status
    later)."""
    torch = _torch()
    gt, ot = _operand_table(groups, "a group table"), _operand_table(operands)
    dev = ot.device
    ft = _operand_table(filters, "a filter table") if filters is not None and len(filters) else None
    if gt.device != dev or (ft is not None and ft.device != dev):
        raise WahError("the filter table, the group table and the operand table are on one device")
    r = int(rows_per_group)
    if r < 1 or gt.shape[0] % r:
        raise WahError("the group table holds rows_per_group >= 1 rows for every group")
    bits = [int(b) for b in attr_bits]
    if not bits or len(bits) > GROUP_MAX_ATTRS or any(b < 1 or b > 64 for b in bits):
        raise WahError("attr_bits: 1 .. 64 widths of 1 .. 64 slices")
    n, f, g, k, a = int(n_words), 0 if ft is None else int(ft.shape[0]), int(gt.shape[0]) // r, int(ot.shape[0]), len(bits)
    if scratch is None:
        scratch = torch.empty(int(lib().wah_select_scratch_bytes(n, k)), dtype=torch.uint8, device=dev)
    group_rows, counts, sums = (
        _int64_tensor(torch, given, shape, dev, f"{name}: a contiguous int64 {list(shape)} tensor on the tables' device")
        for name, given, shape in (("group_rows", group_rows, (g,)), ("counts", counts, (g, k)), ("sums", sums, (g, a, 2))))
    widths = (ctypes.c_uint8 * a)(*bits)
    _enqueued("wah_group_sum_indexed_device", "group_sum",
              lambda *tail: lib().wah_group_sum_indexed_device(n, f, ft.data_ptr() if f else None, g, r, gt.data_ptr(), k, ot.data_ptr(), a, widths,
                                                               group_rows.data_ptr(), counts.data_ptr(), sums.data_ptr(), *tail),
              lib().wah_select_status, scratch, check)
    return group_rows, counts, sums


GROUP_BY_ACCUMULATE = 2  # WAH_GROUP_BY_ACCUMULATE
GROUP_BY_MAX_BUCKETS = 1 << 30  # WAH_GROUP_BY_MAX_BUCKETS


def bsi_group_by_device(key_table, n_words, n_rows, n_buckets, value_table=None, filters=None, exists=False, lookup=None, accumulate=False,
                        scratch=None, counts=None, sums=None, check=True):
    """`SELECT key, COUNT(*), SUM(value) WHERE <filters> GROUP BY key` over a BIT-SLICED key in one call, no bitmap and no value
    column written and nothing read back (wah_bsi_group_by_indexed_device).  key_table: the key's 1 .. 32 slices, most significant
    first, and with exists=True its existence bitmap as one more row behind them; value_table: the value attribute's 1 .. 32 slices,
    most significant first, no existence row, or None: count only; filters: rows ANDed into the selection (None or empty: no
    filter).  The three tables: each a list of (stream, seg_offsets) pairs or a ready [k, 3] table (bitop_operand_table,
    columns.column_operand_table) -- only the device reads them.  Rows at or behind n_rows are never counted.  lookup: a contiguous
    int32 / uint32 device tensor, key -> bucket (a key at or behind its end, and an entry at or above n_buckets -- 0xFFFFFFFF, -1 as
    int32, drops a key -- go to the bucket "other"), or None: the key is the bucket.  Returns (counts [n_buckets + 1], sums
    [n_buckets + 1, 2] or None) as int64 device tensors, "other" last, the sums as low and high 64 bits (bit patterns: a low word
    at or above 2^63 reads as negative).  accumulate=True ADDS into the counts / sums passed in, which are otherwise cleared by the
    call.  scratch / counts / sums: reuse these tensors; check=False: only enqueue (the caller reads wah_bsi_group_by_status
    later)."""
    torch = _torch()
    kt = _operand_table(key_table, "a key table")
    dev = kt.device
    vt = _operand_table(value_table, "a value table") if value_table is not None else None
    ft = _operand_table(filters, "a filter table") if filters is not None and len(filters) else None
    if (vt is not None and vt.device != dev) or (ft is not None and ft.device != dev):
        raise WahError("the filter table, the key table and the value table are on one device")
    if lookup is not None and (not isinstance(lookup, torch.Tensor) or lookup.dtype not in (torch.int32, torch.uint32) or lookup.dim() != 1 or
                               lookup.device != dev or not lookup.is_contiguous() or not lookup.numel()):
        raise WahError("lookup: a contiguous one-dimensional int32 or uint32 tensor of at least one key on the tables' device")
    if accumulate and (counts is None or (vt is not None and sums is None)):
        raise WahError("accumulate=True adds into the counts and sums it is given")
    n, r, b = int(n_words), int(n_rows), int(n_buckets)
    if not 1 <= b <= GROUP_BY_MAX_BUCKETS:
        raise WahError("between 1 and 2^30 buckets")
    ks = int(kt.shape[0]) - (1 if exists else 0)
    vs, f = 0 if vt is None else int(vt.shape[0]), 0 if ft is None else int(ft.shape[0])
    if scratch is None:
        scratch = torch.empty(int(lib().wah_bsi_group_by_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    counts = _int64_tensor(torch, counts, (b + 1,), dev, "counts: a contiguous int64 [n_buckets + 1] tensor on the tables' device")
    if vt is not None:
        sums = _int64_tensor(torch, sums, (b + 1, 2), dev, "sums: a contiguous int64 [n_buckets + 1, 2] tensor on the tables' device")
    elif sums is not None:
        raise WahError("sums go with a value table")
    flags = (BSI_EXISTS if exists else 0) | (GROUP_BY_ACCUMULATE if accumulate else 0)
    _enqueued("wah_bsi_group_by_indexed_device", "bsi_group_by",
              lambda *tail: lib().wah_bsi_group_by_indexed_device(n, r, f, ft.data_ptr() if f else None, ks, kt.data_ptr(), vs,
                                                                  vt.data_ptr() if vs else None, None if lookup is None else lookup.data_ptr(),
                                                                  0 if lookup is None else int(lookup.numel()), b, flags, counts.data_ptr(),
                                                                  sums.data_ptr() if vs else None, *tail),
              lib().wah_bsi_group_by_status, scratch, check)
    return counts, sums


MAP_PARTIAL = 2  # WAH_MAP_PARTIAL
MAP_NULL = 0xFFFFFFFF  # WAH_MAP_NULL


def bsi_map_device(key_table, n_words, n_rows, lookup, n_bits_out, exists=False, partial=False, scratch=None, out=None, out_offsets=None,
                   check=True):
    """A BIT-SLICED key pushed through a lookup table, the looked-up value as a NEW bit-sliced attribute, in one call and with
    nothing read back (wah_bsi_map_indexed_device).  key_table: the key's 1 .. 32 slices, most significant first, and with
    exists=True its existence bitmap as one more row behind them -- a list of (stream, seg_offsets) pairs or a ready [k, 3] table;
    only the device reads it.  lookup: key -> value, a device tensor or a sequence of ints (converted as columns._lookup_tensor
    does: the low 32 bits), at least one entry; MAP_NULL (0xFFFFFFFF, -1 as int32) is "no value", so 2^32 - 1 is not a storable
    value.  n_bits_out: 1 .. 32, the result's slices; an entry with a bit at or above it is refused (WAH_ERR_STREAM).  A row has a
    value when it lies in front of n_rows, exists in the key, its key lies inside the lookup and its entry is not MAP_NULL;
    partial=False refuses (WAH_ERR_STREAM) an existing row in front of n_rows without one, partial=True stores it as 0 outside the
    result's existence bitmap.  The result has an existence bitmap as its last slice exactly when exists or partial.  n_words:
    the words of one slice, a multiple of 992.  Returns as bsi_build_device: (stream, seg_offsets), the slices' compress() streams
    back to back, MOST significant first, and the rows_out * (n_words / 992) + 1 entries of their segment index; scratch / out /
    out_offsets: reuse these tensors; check=False: only enqueue and return (out, count tensor, out_offsets) -- the caller reads
    wah_bsi_map_status later."""
    from .columns import _lookup_tensor

    kt = _operand_table(key_table, "a key table")
    dev = kt.device
    lookup = _lookup_tensor(lookup, dev)
    if not lookup.numel():
        raise WahError("lookup: at least one key")
    n, r, k_out = int(n_words), int(n_rows), int(n_bits_out)
    ks = int(kt.shape[0]) - (1 if exists else 0)
    if not (1 <= ks <= 32 and 1 <= k_out <= 32):
        raise WahError("a key of 1 to 32 slices and a result of 1 to 32")
    if n <= 0 or n % 992:
        raise WahError("slices of a multiple of 992 words")
    flags = (BSI_EXISTS if exists else 0) | (MAP_PARTIAL if partial else 0)
    rows_out = k_out + (1 if flags else 0)
    n_keys = int(lookup.numel())
    # (the lookup converted here lives until the call is enqueued: the stream keeps its memory valid for the launches behind it)
    return _compressed_streams(
        "wah_bsi_map_indexed_device", "bsi_map", dev, rows_out * (n // 992) + 1, _ROWS_OUT_OFFSETS,
        lambda: lib().wah_bsi_map_scratch_bytes(n, k_out, flags), lambda: max_compressed_words(rows_out * n),
        lambda *tail: lib().wah_bsi_map_indexed_device(n, r, ks, kt.data_ptr(), lookup.data_ptr(), n_keys, k_out, flags, *tail),
        lambda sc, sp: lib().wah_bsi_map_status(sc, n, k_out, flags, sp), scratch, out, out_offsets, check)


CUMSUM_EXCLUSIVE = 2  # WAH_CUMSUM_EXCLUSIVE
CUMSUM_ALL_ROWS = 4  # WAH_CUMSUM_ALL_ROWS


def bsi_cumsum_device(val_table, n_words, n_rows, n_bits_val, n_bits_out, filters=None, exists=False, exclusive=False, all_rows=False,
                      scratch=None, out=None, out_offsets=None, check=True):
    """The RUNNING SUM of a bit-sliced value over the rows that the filters select, as a NEW bit-sliced attribute, in one call and
    with nothing read back (wah_bsi_cumsum_indexed_device): `SUM(x) OVER (ORDER BY rowid) ... WHERE f`, and with n_bits_val == 0
    the running COUNT, ROW_NUMBER() over the selected rows.  val_table: the value's n_bits_val slices (0 .. 32), most significant
    first, unsigned, and with exists=True its existence bitmap as one more row behind them -- a list of (stream, seg_offsets) pairs
    or a ready [k, 3] table, None when it has no row at all; filters: rows ANDed into the selection (None or empty: no filter).
    Only the device reads the tables.  A row is selected when it lies in front of n_rows, is set in every filter row and, with
    exists=True, in the existence bitmap.  Row p of the result holds the sum of the values of the selected rows q <= p
    (exclusive=True: q < p) mod 2^n_bits_out, n_bits_out 1 .. 64; the sum is carried in 64 bits and cut where it is stored.
    all_rows=False: only selected rows hold a value, every other row is 0, and the result's last slice is its existence bitmap,
    the selection; all_rows=True: every row in front of n_rows holds the running value, unselected rows carrying it forward, and
    the result has no existence bitmap.  n_words: the words of one slice, a multiple of 992.  Returns as bsi_build_device:
    (stream, seg_offsets), the slices' compress() streams back to back, MOST significant first, and the rows_out * (n_words / 992)
    + 1 entries of their segment index, rows_out = n_bits_out + (0 if all_rows else 1); scratch / out / out_offsets: reuse these
    tensors; check=False: only enqueue and return (out, count tensor, out_offsets) -- the caller reads wah_bsi_cumsum_status
    later."""
    n, r, kv, k_out = int(n_words), int(n_rows), int(n_bits_val), int(n_bits_out)
    if not (0 <= kv <= 32 and 1 <= k_out <= 64):
        raise WahError("a value of 0 to 32 slices and a result of 1 to 64")
    if n <= 0 or n % 992:
        raise WahError("slices of a multiple of 992 words")
    vt = _operand_table(val_table, "a value table") if kv or exists else None
    ft = _operand_table(filters, "a filter table") if filters is not None and len(filters) else None
    if vt is None and ft is None:
        raise WahError("without value slices and without an existence bitmap the call needs a filter: its device is the call's")
    if vt is not None and int(vt.shape[0]) != kv + (1 if exists else 0):
        raise WahError("a value table of n_bits_val rows, and one more with exists=True")
    if vt is not None and ft is not None and vt.device != ft.device:
        raise WahError("the filter table and the value table are on one device")
    dev = vt.device if vt is not None else ft.device
    f = 0 if ft is None else int(ft.shape[0])
    flags = (BSI_EXISTS if exists else 0) | (CUMSUM_EXCLUSIVE if exclusive else 0) | (CUMSUM_ALL_ROWS if all_rows else 0)
    rows_out = k_out + (0 if all_rows else 1)
    return _compressed_streams(
        "wah_bsi_cumsum_indexed_device", "bsi_cumsum", dev, rows_out * (n // 992) + 1, _ROWS_OUT_OFFSETS,
        lambda: lib().wah_bsi_cumsum_scratch_bytes(n, k_out, flags), lambda: max_compressed_words(rows_out * n),
        lambda *tail: lib().wah_bsi_cumsum_indexed_device(n, r, f, ft.data_ptr() if f else None, kv, None if vt is None else vt.data_ptr(), k_out,
                                                          flags, *tail),
        lambda sc, sp: lib().wah_bsi_cumsum_status(sc, n, k_out, flags, sp), scratch, out, out_offsets, check)


def bsi_cumsum_parts_device(val_table, n_words, n_rows, n_bits_val, n_bits_out, starts, filters=None, exists=False, exclusive=False,
                            all_rows=False, scratch=None, out=None, out_offsets=None, check=True):
    """The RUNNING SUM PER PARTITION (wah_bsi_cumsum_parts_indexed_device): bsi_cumsum_device with a sum that starts again at
    every row set in `starts` -- `SUM(x) OVER (PARTITION BY g ORDER BY rowid) ... WHERE f` on a table clustered by g, and with
    n_bits_val == 0 ROW_NUMBER() OVER (PARTITION BY g).  starts: ONE indexed bitmap of n_words words, a one-row operand table or a
    (stream, seg_offsets) pair; row p starts a partition when its bit is set and p < n_rows, selected or not.  Row p of the result
    holds the sum of the values of the selected rows q with s(p) <= q <= p (exclusive=True: q < p), s(p) the last start at or in
    front of p, row 0 without one.  Everything else -- tables, flags, the result, scratch / out / out_offsets / check -- as
    bsi_cumsum_device; the status call is wah_bsi_cumsum_parts_status."""
    flags = (BSI_EXISTS if exists else 0) | (CUMSUM_EXCLUSIVE if exclusive else 0) | (CUMSUM_ALL_ROWS if all_rows else 0)
    return _bsi_parts_call("bsi_cumsum_parts", val_table, n_words, n_rows, n_bits_val, n_bits_out, starts, filters, exists, flags, all_rows,
                           scratch, out, out_offsets, check)


def _bsi_parts_call(name, val_table, n_words, n_rows, n_bits_val, n_bits_out, starts, filters, exists, flags, all_rows, scratch, out, out_offsets,
                    check):
    """bsi_cumsum_parts_device's and bsi_total_parts_device's road: the argument checks, the three tables and the call
    wah_<name>_indexed_device with its scratch_bytes and status calls."""
    n, r, kv, k_out = int(n_words), int(n_rows), int(n_bits_val), int(n_bits_out)
    if not (0 <= kv <= 32 and 1 <= k_out <= 64):
        raise WahError("a value of 0 to 32 slices and a result of 1 to 64")
    if n <= 0 or n % 992:
        raise WahError("slices of a multiple of 992 words")
    if isinstance(starts, tuple) and len(starts) == 2:
        starts = [starts]
    st = _operand_table(starts, "a starts row")
    if int(st.shape[0]) != 1:
        raise WahError("a starts table of one row")
    vt = _operand_table(val_table, "a value table") if kv or exists else None
    ft = _operand_table(filters, "a filter table") if filters is not None and len(filters) else None
    if vt is not None and int(vt.shape[0]) != kv + (1 if exists else 0):
        raise WahError("a value table of n_bits_val rows, and one more with exists=True")
    if any(t is not None and t.device != st.device for t in (vt, ft)):
        raise WahError("the starts row, the filter table and the value table are on one device")
    f = 0 if ft is None else int(ft.shape[0])
    rows_out = k_out + (0 if all_rows else 1)
    call, size, status = (getattr(lib(), f"wah_{name}_{tail}") for tail in ("indexed_device", "scratch_bytes", "status"))
    return _compressed_streams(
        f"wah_{name}_indexed_device", name, st.device, rows_out * (n // 992) + 1, _ROWS_OUT_OFFSETS,
        lambda: size(n, k_out, flags), lambda: max_compressed_words(rows_out * n),
        lambda *tail: call(n, r, f, ft.data_ptr() if f else None, kv, None if vt is None else vt.data_ptr(), st.data_ptr(), k_out, flags, *tail),
        lambda sc, sp: status(sc, n, k_out, flags, sp), scratch, out, out_offsets, check)


def bsi_total_parts_device(val_table, n_words, n_rows, n_bits_val, n_bits_out, starts, filters=None, exists=False, all_rows=False, scratch=None,
                           out=None, out_offsets=None, check=True):
    """The PARTITION'S TOTAL IN EVERY ROW (wah_bsi_total_parts_indexed_device): `SUM(x) OVER (PARTITION BY g) ... WHERE f` on a table
    clustered by g, and with n_bits_val == 0 COUNT(*) OVER (PARTITION BY g).  starts as bsi_cumsum_parts_device's.  Row p of the
    result holds the sum of the values of the selected rows from s(p), the last start at or in front of p (row 0 without one), up to
    the row in front of the next start behind p (the last row in front of n_rows without one); with all_rows=True every row in
    front of n_rows holds it, otherwise the selected ones.  No start at all: the grand total in every row.  Everything else --
    tables, exists, the result, scratch / out / out_offsets / check -- as bsi_cumsum_parts_device; there is no exclusive form; the
    status call is wah_bsi_total_parts_status."""
    flags = (BSI_EXISTS if exists else 0) | (CUMSUM_ALL_ROWS if all_rows else 0)
    return _bsi_parts_call("bsi_total_parts", val_table, n_words, n_rows, n_bits_val, n_bits_out, starts, filters, exists, flags, all_rows, scratch,
                           out, out_offsets, check)


def positions_device(stream, seg_offsets, n_words, first=0, limit=None, out=None, scratch=None, check=True):
    """The positions (row numbers) of the set bits of one indexed compressed bitmap, ascending, without decoding it
    (wah_positions_indexed_device): those of ranks [first, first + limit).  Returns (positions int64 tensor, total set bits).
    With limit=None TWO calls are made: the first one asks for the total only, the second one writes into an output of
    exactly total - first entries.  out: write into this int64 tensor (its length is the limit when none is given);
    scratch: reuse this tensor.  check=False (needs a limit or an out): only enqueue and return (out, info tensor) with
    info = [total, number written]."""
    torch = _torch()
    _as_words(torch, stream)
    if seg_offsets.dtype != torch.int64 or not seg_offsets.is_cuda or not seg_offsets.is_contiguous():
        raise WahError("a segment index is a contiguous int64 CUDA tensor")
    dev = stream.device
    n, first = int(n_words), int(first)
    if first < 0 or (limit is not None and int(limit) < 0):
        raise WahError("first and limit are not negative")
    if scratch is None:
        scratch = torch.empty(int(lib().wah_select_scratch_bytes(n, 1)), dtype=torch.uint8, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    sp = _stream_ptr(torch)

    def call(dst, cap):
        _check(lib().wah_positions_indexed_device(n, stream.data_ptr(), stream.numel(), seg_offsets.data_ptr(), first,
                                                  dst.data_ptr() if cap else None, cap, info.data_ptr(), scratch.data_ptr(),
                                                  scratch.numel(), sp), "wah_positions_indexed_device")

    if out is not None:  # (one-dimensional, of whatever length)
        _int64_tensor(torch, out, (out.numel(),), dev, "out: a contiguous one-dimensional int64 tensor on the stream's device")
        limit = int(out.numel()) if limit is None else min(int(limit), int(out.numel()))
    if limit is None:
        if not check:
            raise WahError("check=False needs a limit or an out: the output's size comes from a first, checked call")
        call(info, 0)
        _check(lib().wah_select_status(scratch.data_ptr(), sp), "positions")
        limit = max(int(info[0].item()) - first, 0)
    limit = int(limit)
    if out is None:
        out = torch.empty(limit, dtype=torch.int64, device=dev)
    call(out, limit)
    if not check:
        return out, info
    _check(lib().wah_select_status(scratch.data_ptr(), sp), "positions")
    total, written = (int(v) for v in info.tolist())
    return out[:written], total


def from_positions_max_words(n_words, n_lists, n_rows):
    return int(lib().wah_from_positions_max_words(int(n_words), int(n_lists), int(n_rows)))


def from_positions_device(rows, list_ends, n_words, scratch=None, out=None, out_offsets=None, check=True):
    """Compressed bitmaps of n_words words straight from sorted lists of row numbers, any number of lists in one call and no
    decoded bitmap (wah_from_positions_device).  rows: a contiguous int64 CUDA tensor, the lists back to back, each strictly
    ascending and below 32 * n_words; list_ends: a contiguous int64 CUDA tensor on the same device, one past every list's last
    row (never decreasing, the last one len(rows)) -- only the device reads them.  Returns (stream, seg_offsets): the lists'
    compress() streams back to back and the n_lists * S + 1 entries of their segment index (S = segments of one bitmap); list c
    is the operand (stream, seg_offsets[c * S:]).  scratch / out / out_offsets: reuse these tensors (out defaults to
    wah_from_positions_max_words words); check=False: only enqueue and return (out, count tensor, out_offsets)."""
    torch = _torch()
    for t, what in ((rows, "rows"), (list_ends, "list_ends")):
        if t.dtype != torch.int64 or t.dim() != 1 or not t.is_cuda or not t.is_contiguous():
            raise WahError(f"{what}: a contiguous one-dimensional int64 CUDA tensor")
    if list_ends.device != rows.device or list_ends.numel() < 1:
        raise WahError("list_ends: at least one entry, on the rows' device")
    dev = rows.device
    n, k, r = int(n_words), int(list_ends.numel()), int(rows.numel())
    n_seg = (max_compressed_words(n) + 1023) // 1024
    return _compressed_streams(
        "wah_from_positions_device", "from_positions", dev, k * n_seg + 1,
        "out_offsets: a contiguous int64 tensor of n_lists * segments + 1 entries on the rows' device",
        lambda: lib().wah_from_positions_scratch_bytes(n, k), lambda: max(from_positions_max_words(n, k, r), 1),
        lambda *tail: lib().wah_from_positions_device(n, k, list_ends.data_ptr(), rows.data_ptr() if r else None, r, *tail),
        lib().wah_from_positions_status, scratch, out, out_offsets, check)


SPLICE_MAX_PIECES = 1 << 16  # WAH_SPLICE_MAX_PIECES


def splice_pieces(pieces, device=None):
    """The wah_splice_piece array of a list of (n_words, first_row, n_rows) triples as an int64 device tensor of shape
    [n_pieces, 3] (splice_device)."""
    torch = _torch()
    rows = [(int(n), int(f), int(r)) for n, f, r in pieces]
    if not rows or any(v < 0 for row in rows for v in row):
        raise WahError("at least one piece of (n_words, first_row, n_rows), none of them negative")
    return torch.tensor(rows, dtype=torch.int64, device="cuda" if device is None else device)


def splice_max_words(n_words_out, n_columns, n_pieces, source_words):
    return int(lib().wah_splice_max_words(int(n_words_out), int(n_columns), int(n_pieces), int(source_words)))


def splice_device(pieces, table, n_columns, n_words_out, source_words=None, scratch=None, out=None, out_offsets=None, check=True):
    """Row ranges of indexed compressed bitmaps concatenated into new ones, at any bit offset, for n_columns columns at once and
    without a decoded bitmap (wah_splice_indexed_device).  pieces: the [n_pieces, 3] int64 table of splice_pieces, or a list of
    (n_words, first_row, n_rows) triples; table: the [n_pieces * n_columns, 3] operand table (bitop_operand_table,
    columns.column_operand_table), piece-major: row p * n_columns + c is column c of piece p -- only the device reads either.
    Output column c holds, piece after piece, positions first_row .. first_row + n_rows of the pieces' column c, and zeros behind
    them, in n_words_out words.  Returns (stream, seg_offsets): the columns' compress() streams back to back and the
    n_columns * S + 1 entries of their segment index (S = segments of one output bitmap), as from_positions_device.
    source_words: an upper bound on the words of the source segments that are read, which sizes a default out by
    wah_splice_max_words (None: the bound that always holds, n_columns * wah_max_compressed_words(n_words_out));
    scratch / out / out_offsets: reuse these tensors; check=False: only enqueue and return (out, count tensor, out_offsets)."""
    torch = _torch()
    table = _operand_table(table)
    dev = table.device
    if not isinstance(pieces, torch.Tensor):
        pieces = splice_pieces(pieces, dev)
    if pieces.dtype != torch.int64 or pieces.dim() != 2 or pieces.shape[1] != 3 or pieces.shape[0] < 1 or not pieces.is_contiguous() or pieces.device != dev:
        raise WahError("pieces: a contiguous int64 tensor of shape [n_pieces, 3] on the table's device")
    n, k, p = int(n_words_out), int(n_columns), int(pieces.shape[0])
    if k < 1 or int(table.shape[0]) != p * k:
        raise WahError("the operand table holds n_columns >= 1 rows for every piece")
    n_seg = (max_compressed_words(n) + 1023) // 1024
    return _compressed_streams(
        "wah_splice_indexed_device", "splice", dev, k * n_seg + 1,
        "out_offsets: a contiguous int64 tensor of n_columns * segments + 1 entries on the table's device",
        lambda: lib().wah_splice_scratch_bytes(n, k, p),
        lambda: max(k * max_compressed_words(n) if source_words is None else splice_max_words(n, k, p, source_words), 1),
        lambda *tail: lib().wah_splice_indexed_device(n, k, p, pieces.data_ptr(), table.data_ptr(), *tail),
        lib().wah_splice_status, scratch, out, out_offsets, check)


COMPACT_DELETE = 1  # WAH_COMPACT_DELETE


def compact_max_words(n_words_out, n_columns, source_words):
    return int(lib().wah_compact_max_words(int(n_words_out), int(n_columns), int(source_words)))


def compact_device(mask, table, n_words, n_rows, n_words_out, delete=False, source_words=None, scratch=None, out=None, out_offsets=None,
                   out_rows=None, check=True):
    """The rows a mask bitmap selects of every column of an index moved together into new indexed bitmaps, without a decoded
    bitmap (wah_compact_indexed_device).  mask: a (stream, seg_offsets) pair or a ready [1, 3] operand table; table: the
    [n_columns, 3] operand table of the columns (bitop_operand_table, columns.column_operand_table), or a list of pairs -- all
    bitmaps of n_words words, only the device reads them.  Only positions below n_rows are rows.  A row is selected where its
    mask bit is 1, with delete=True where it is 0; output column c holds column c's bits at the selected rows, in order, and
    zeros behind them, in n_words_out words.  Returns (stream, seg_offsets, rows): the columns' compress() streams back to back,
    the n_columns * S + 1 entries of their segment index (S = segments of one output bitmap), as splice_device, and a
    one-element int64 device tensor that holds the number of selected rows.  source_words: an upper bound on the words of the
    column segments that are read, which sizes a default out by wah_compact_max_words (None: the bound that always holds,
    n_columns * wah_max_compressed_words(n_words_out)); scratch / out / out_offsets / out_rows: reuse these tensors;
    check=False: only enqueue and return (out, count tensor, out_offsets, rows)."""
    torch = _torch()
    table = _operand_table(table)
    dev = table.device
    if not isinstance(mask, torch.Tensor):
        mask = [tuple(mask)]
    mask = _operand_table(mask, "the mask")
    if int(mask.shape[0]) != 1 or mask.device != dev:
        raise WahError("the mask is one operand on the table's device")
    n, r, n_out, k = int(n_words), int(n_rows), int(n_words_out), int(table.shape[0])
    if r < 0 or r > 32 * n:
        raise WahError("n_rows lies between 0 and 32 * n_words")
    rows = _int64_tensor(torch, out_rows, (1,), dev, "out_rows: a contiguous int64 tensor of one entry on the table's device")
    flags = COMPACT_DELETE if delete else 0
    n_seg = (max_compressed_words(n_out) + 1023) // 1024
    got = _compressed_streams(
        "wah_compact_indexed_device", "compact", dev, k * n_seg + 1,
        "out_offsets: a contiguous int64 tensor of n_columns * segments + 1 entries on the table's device",
        lambda: lib().wah_compact_scratch_bytes(n, n_out, k),
        lambda: max(k * max_compressed_words(n_out) if source_words is None else compact_max_words(n_out, k, source_words), 1),
        lambda *tail: lib().wah_compact_indexed_device(n, r, flags, mask.data_ptr(), k, table.data_ptr(), n_out, *tail[:4], rows.data_ptr(), *tail[4:]),
        lib().wah_compact_status, scratch, out, out_offsets, check)
    return got + (rows,)


def update_operand_table(entries, device=None):
    """The wah_bitop_operand array of the else or the then side of update_device, as an int64 device tensor of shape [k, 3]: every
    entry is a (stream, seg_offsets) pair, which becomes the row of bitop_operand_table, or the int 0 or 1, a CONSTANT bitmap of
    that bit, which becomes the row (0, bit, 0) -- no stream, no index, nothing is read for it.  As bitop_operand_table the table
    holds raw pointers and keeps no tensor alive.  device: where the table goes; needed when every entry is a constant."""
    torch = _torch()
    if not entries:
        raise WahError("an operand table needs at least one operand")
    rows, dev = [], device
    for e in entries:
        if isinstance(e, (tuple, list)):
            st, offs = e
            _as_words(torch, st)
            if offs.dtype != torch.int64 or not offs.is_cuda or not offs.is_contiguous():
                raise WahError("a segment index is a contiguous int64 CUDA tensor")
            rows.append((st.data_ptr(), st.numel(), offs.data_ptr()))
            if dev is None:
                dev = st.device
        elif e in (0, 1):
            rows.append((0, int(e), 0))
        else:
            raise WahError("an entry is a (stream, seg_offsets) pair or the constant 0 or 1")
    if dev is None:
        raise WahError("a table of constants only needs a device")
    return torch.tensor(rows, dtype=torch.int64, device=dev)


def update_max_words(n_words, n_columns, mask_words, source_words):
    return int(lib().wah_update_max_words(int(n_words), int(n_columns), int(mask_words), int(source_words)))


def update_device(mask, else_table, then_table, n_words, n_rows, mask_words=None, source_words=None, scratch=None, out=None,
                  out_offsets=None, check=True):
    """Per column the blend of two indexed bitmaps under a mask bitmap, without a decoded bitmap (wah_update_indexed_device):
    output column c is then_table's row c where the mask bit is 1 and the position lies below n_rows, else_table's row c
    everywhere else.  mask: a (stream, seg_offsets) pair or a ready [1, 3] operand table; else_table / then_table: [n_columns, 3]
    operand tables (update_operand_table, bitop_operand_table, columns.column_operand_table) or lists of update_operand_table's
    entries -- all bitmaps of n_words words, only the device reads them; a row (0, bit, 0) is a constant.  Returns
    (stream, seg_offsets): the columns' compress() streams back to back and the n_columns * S + 1 entries of their segment index,
    as compact_device.  mask_words / source_words: upper bounds on the mask's words and on the words of all else and then rows
    that are no constants together, which size a default out by wah_update_max_words (either None: the bound that always holds,
    n_columns * wah_max_compressed_words(n_words)); scratch / out / out_offsets: reuse these tensors; check=False: only enqueue
    and return (out, count tensor, out_offsets).  The output must not overlap an input."""
    torch = _torch()
    if not isinstance(mask, torch.Tensor):
        mask = [tuple(mask)]
    mask = _operand_table(mask, "the mask")
    dev = mask.device

    def side(x, what):
        return _operand_table(x if isinstance(x, torch.Tensor) else update_operand_table(x, dev), what)

    else_table, then_table = side(else_table, "the else table"), side(then_table, "the then table")
    k = int(else_table.shape[0])
    if int(mask.shape[0]) != 1 or int(then_table.shape[0]) != k or else_table.device != dev or then_table.device != dev:
        raise WahError("the mask is one operand, the else and the then table have one row per column, all on one device")
    n, r = int(n_words), int(n_rows)
    if r < 0 or r > 32 * n:
        raise WahError("n_rows lies between 0 and 32 * n_words")
    g = max_compressed_words(n)
    exact = mask_words is not None and source_words is not None
    return _compressed_streams(
        "wah_update_indexed_device", "update", dev, k * ((g + 1023) // 1024) + 1,
        "out_offsets: a contiguous int64 tensor of n_columns * segments + 1 entries on the table's device",
        lambda: lib().wah_update_scratch_bytes(n, k),
        lambda: max(update_max_words(n, k, mask_words, source_words) if exact else k * g, 1),
        lambda *tail: lib().wah_update_indexed_device(n, r, mask.data_ptr(), k, else_table.data_ptr(), then_table.data_ptr(), *tail),
        lib().wah_update_status, scratch, out, out_offsets, check)


def bsi_build_device(values, n_bits, n_words, exists=None, scratch=None, out=None, out_offsets=None, check=True):
    """The bit-sliced index of a value column in one call (wah_bsi_build_device): the column is transposed into its decoded slice
    matrix on the device and that is compressed as one bitmap.  values: a contiguous one-dimensional int64 CUDA tensor, read as
    UNSIGNED, every value below 2^n_bits, n_bits 1 .. 64; exists: a torch.bool tensor of the same length on the same device -- a
    row without a value is stored as 0 and the existence bitmap becomes the last slice -- or None; only the device reads either.
    n_words: the words of one slice, a multiple of 992 that holds every row.  Returns (stream, seg_offsets): the slices'
    compress() streams back to back, MOST significant slice first, and the n_slices * (n_words / 992) + 1 entries of their
    segment index; slice i is the operand (stream, seg_offsets[i * (n_words // 992):]), and the pair goes into
    columns.column_operand_table as a column matrix's does.  scratch / out / out_offsets: reuse these tensors (out defaults to
    wah_max_compressed_words(n_slices * n_words) words); check=False: only enqueue and return (out, count tensor, out_offsets)
    -- the caller reads wah_bsi_build_status later."""
    torch = _torch()
    if values.dtype != torch.int64 or values.dim() != 1 or not values.is_cuda or not values.is_contiguous():
        raise WahError("values: a contiguous one-dimensional int64 CUDA tensor")
    dev = values.device
    n, bits, r = int(n_words), int(n_bits), int(values.numel())
    if exists is not None and (exists.dtype != torch.bool or tuple(exists.shape) != (r,) or exists.device != dev or not exists.is_contiguous()):
        raise WahError("exists: a contiguous torch.bool tensor of the values' length on their device")
    if not 1 <= bits <= 64 or n <= 0 or n % 992:
        raise WahError("between 1 and 64 bits, slices of a multiple of 992 words")
    k = bits + (exists is not None)
    # (an empty bool tensor still stands for "with an existence bitmap": the library tells by the pointer, so it gets the scratch's,
    # tail[4])
    return _compressed_streams(
        "wah_bsi_build_device", "bsi_build", dev, k * (n // 992) + 1,
        "out_offsets: a contiguous int64 tensor of n_slices * n_words / 992 + 1 entries on the values' device",
        lambda: lib().wah_bsi_build_scratch_bytes(n, k), lambda: max_compressed_words(k * n),
        lambda *tail: lib().wah_bsi_build_device(n, bits, values.data_ptr() if r else None, r,
                                                 None if exists is None else exists.data_ptr() if r else tail[4], *tail),
        lambda sc, sp: lib().wah_bsi_build_status(sc, n, k, sp), scratch, out, out_offsets, check)


StreamReport = collections.namedtuple(
    "StreamReport", "groups words empty_fills fillable_literals crossing_fills unmerged_fills segment_canonical")


def validate_device(d_comp):
    """What a compressed stream contains (include/wah.h: wah_validate_device), without decoding it."""
    torch = _torch()
    _as_words(torch, d_comp)
    c = int(d_comp.numel())
    ws_bytes = int(lib().wah_decompress_workspace_bytes(c, 0))
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=d_comp.device)
    report = torch.zeros(8, dtype=torch.int64, device=d_comp.device)
    _check(lib().wah_validate_device(d_comp.data_ptr(), c, report.data_ptr(), ws.data_ptr(), ws_bytes, _stream_ptr(torch)),
           "wah_validate_device")
    _check(lib().wah_decompress_status(ws.data_ptr(), _stream_ptr(torch)), "validate")
    r = report.cpu().tolist()
    return StreamReport(r[0], r[1], r[2], r[3], r[4], r[5], bool(r[6]))


def gen_uniform_device(n_words, seed, p, device="cuda:0", out=None):
    """Bernoulli(p) bitmap generated in HBM (bit-exact definition: include/wah_gen.h); `out`: write into this tensor."""
    torch = _torch()
    if out is None:
        out = torch.empty(max(int(n_words), 1), dtype=torch.int32, device=device)
    else:
        _as_words(torch, out)
    _check(lib().wah_gen_uniform_device(out.data_ptr(), int(n_words), int(seed), threshold_for(p),
                                        _stream_ptr(torch)), "wah_gen_uniform_device")
    return out[: int(n_words)]


def gen_clustered_device(n_words, seed, mean_run_bits=4096, device="cuda:0", out=None):
    torch = _torch()
    if out is None:
        out = torch.empty(max(int(n_words), 1), dtype=torch.int32, device=device)
    else:
        _as_words(torch, out)
    _check(lib().wah_gen_clustered_device(out.data_ptr(), int(n_words), int(seed), threshold_for(1.0 / mean_run_bits),
                                          _stream_ptr(torch)), "wah_gen_clustered_device")
    return out[: int(n_words)]


def copy_device(d_in, d_out):
    torch = _torch()
    _check(lib().wah_copy_device(d_in.data_ptr(), d_out.data_ptr(), int(d_in.numel()), _stream_ptr(torch)),
           "wah_copy_device")

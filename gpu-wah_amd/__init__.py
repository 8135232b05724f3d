"""wah-mi355x: MI355X-native WAH bitmap compressor / decompressor.

Host-side mirror of the reference's operator interface for this path:

    compress(data)   <->  compress()   /root/reference/compress.h:12-18, compress.cu:41-209
    decompress(comp) <->  decompress() /root/reference/decompress.h:11-17, decompress.cu:18-141

Same argument meaning (host buffers of 32-bit words in, a new host buffer out,
sizes in words, three millisecond timings) and the same error behaviour (a
failed call returns nothing usable: here it raises WahError where the reference
returns NULL).  Everything is computed by the HIP library `libwah_hip.so`
through its C ABI (include/wah.h); there is NO CPU fallback -- importing works
without a GPU (so the ABI can be inspected), but every compute call fails
loudly if the library or the device is missing.

The directory name contains a hyphen, so import it with
    importlib.import_module("gpu-wah_amd")
or through the `gpu_wah_amd` shim module at the repository root.
"""
from . import columns  # noqa: F401
from . import report  # noqa: F401
from .api import (  # noqa: F401
    WahError,
    Timings,
    lib,
    lib_path,
    build,
    compress,
    decompress,
    host_cache_release,
    max_compressed_words,
    decoded_words,
    compress_device,
    decompress_device,
    decompress_segments_device,
    build_index_device,
    DeviceCompressor,
    DeviceDecompressor,
    validate_device,
    bitop_device,
    bitop_indexed_device,
    bitop_many_indexed_device,
    bitop_list_indexed_device,
    bitop_operand_table,
    BitopOperand,
    bitop_clauses_indexed_device,
    bitop_clause_table,
    CLAUSE_NEGATE,
    bsi_range_device,
    bsi_bounds,
    BSI_MAX_SLICES,
    BSI_EXISTS,
    bsi_member_device,
    member_set,
    MEMBER_NEGATE,
    MEMBER_BITSET,
    bsi_compare_device,
    bsi_compare_row_order,
    BSI_EXISTS_A,
    BSI_EXISTS_B,
    CMP_OPS,
    bsi_arith_device,
    bsi_arith_row_order,
    ARITH_OPS,
    bsi_mul_device,
    bsi_mul_row_order,
    bsi_kth_device,
    bsi_kth_query,
    BSI_KTH_ASCENDING,
    BSI_KTH_DESCENDING,
    BSI_KTH_QUANTILE,
    BSI_KTH_MAX_FILTERS,
    bsi_kth_grouped_device,
    bsi_kth_queries,
    BSI_KTH_GROUPED_MAX_LANES,
    fetch_device,
    FETCH_BITS,
    FETCH_FIRST,
    values_device,
    count_device,
    count_masked_device,
    group_sum_device,
    GROUP_MAX_FILTERS,
    GROUP_MAX_ROWS,
    GROUP_MAX_ATTRS,
    bsi_group_by_device,
    GROUP_BY_ACCUMULATE,
    GROUP_BY_MAX_BUCKETS,
    bsi_map_device,
    MAP_PARTIAL,
    MAP_NULL,
    positions_device,
    from_positions_device,
    from_positions_max_words,
    splice_device,
    splice_pieces,
    splice_max_words,
    SPLICE_MAX_PIECES,
    compact_device,
    compact_max_words,
    COMPACT_DELETE,
    update_device,
    update_operand_table,
    update_max_words,
    bsi_build_device,
    merge_fills_device,
    StreamReport,
    gen_uniform_device,
    gen_clustered_device,
    copy_device,
    threshold_for,
    version,
    ABI_SYMBOLS,
)

"""Loader for libfltee_agg.so (the HIP library behind include/fltee_agg.h).

The product path has no CPU fallback: if the library is missing the import of
any compute entry point raises.  Build it with `make -C fl-tee_amd` (or
`__graft_entry__.build()`).
"""
import ctypes
import os

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# FLTEE_LIB: another build of the same library (A/B runs of two builds, scripts/ab_env.py)
LIB_PATH = os.environ.get("FLTEE_LIB") or os.path.join(PKG_ROOT, "lib", "libfltee_agg.so")

# include/fltee_agg.h
SUCCESS = 0x0
ERROR_UNEXPECTED = 0x1
ERROR_INVALID_PARAMETER = 0x2
ERROR_OUT_OF_MEMORY = 0x3
ERROR_INVALID_ENCLAVE_ID = 0x2002
ERROR_MAC_MISMATCH = 0x3001  # an authenticated upload's GCM tag did not verify

ALG_ADVANCED, ALG_NIPS19, ALG_BASELINE, ALG_NON_OBLIVIOUS, ALG_PATH_ORAM, ALG_OPTIMIZED = 1, 2, 3, 4, 5, 6
ALG_BUBBLE = 7  # lib.rs:389 (the reference bench's `-a bubble`; not in option.py, not in ALG_CODES)
ALG_CODES = {  # src/option.py:131-145
    "advanced": ALG_ADVANCED, "nips19": ALG_NIPS19, "baseline": ALG_BASELINE,
    "non_oblivious": ALG_NON_OBLIVIOUS, "path_oram": ALG_PATH_ORAM, "optimized": ALG_OPTIMIZED,
}

DEV_ERR_DENSE_ORDER = 0x1
DEV_ERR_INDEX_RANGE = 0x2
DEV_ERR_FOLD_OVERFLOW = 0x4  # retired in round 6: never set
DEV_ERR_AUTH = 0x10

# authenticated uploads (AES-128-GCM; k_ghash.hip)
GCM_SEGMENT_BLOCKS = 512  # FLTEE_GCM_SEGMENT_BLOCKS: 16-byte blocks per GHASH segment
GCM_TAG_BYTES = 16
GCM_MAX_AAD = 64
# fltee_set_upload_aead_policy: what an authenticated ECALL does after a failed tag
AEAD_ABORT, AEAD_REPORT, AEAD_DROP = 0, 1, 2

OPT_DENSE = 0x1
OPT_DP = 0x2
OPT_CLIP = 0x4
OPT_ACCUMULATE = 0x8
OPT_NO_AVERAGE = 0x10
OPT_K_REQ = 0x20
OPT_ORAM_TREE = 0x40
OPT_ORAM_LAZY = 0x80
OPT_PACKED = 0x100  # d_records: packed dense slices (value-only rows of 2 * ceil(d / 2) f32)
OPT_TRIM = 0x200  # coordinate-wise trimmed mean of a dense call, DeviceOpts.trim clients a side
TRIM_MAX = 64  # FLTEE_TRIM_MAX
AAD_PACKED_BIT = 0x80000000  # FLTEE_AAD_PACKED_BIT: a packed call's last AAD word is alg | this
OPT_BF16 = 0x400  # d_records: bf16 dense slices (value-only rows of 4 * ceil(d / 4) bf16)
AAD_BF16_BIT = 0x40000000  # FLTEE_AAD_BF16_BIT: a bf16 call's last AAD word is alg | this
OPT_FP8 = 0x1000  # d_records: fp8 dense slices (8 * (ceil(d / 8) + 1) bytes: e4m3fn codes, then the f32 scale)
AAD_FP8_BIT = 0x20000000  # FLTEE_AAD_FP8_BIT: an fp8 call's last AAD word is alg | this
OPT_TRIM_SELECT = 0x800  # with OPT_TRIM: trim by selection (k_trim_select.hip), any trim with 2 * trim < n
TRIM_SELECT_MAX_N = 4096  # FLTEE_TRIM_SELECT_MAX_N
OPT_KRUM = 0x2000  # Multi-Krum of a dense call (k_krum.hip): DeviceOptsKrum.krum_f assumed Byzantine, krum_m kept
KRUM_MAX_N = 1024  # FLTEE_KRUM_MAX_N
OPT_GMED = 0x4000  # the geometric median of a dense call (k_gmed.hip): DeviceOptsGmed.gmed_iters Weiszfeld iterations, floor gmed_nu
GMED_MAX_ITERS = 64  # FLTEE_GMED_MAX_ITERS


class DeviceOpts(ctypes.Structure):
    """struct fltee_device_opts."""
    _fields_ = [
        ("flags", ctypes.c_uint32),
        ("sigma", ctypes.c_float),
        ("clipping", ctypes.c_float),
        ("seed", ctypes.c_uint64),
        ("k_req", ctypes.c_size_t),
        ("batch", ctypes.c_size_t),
        ("n_avg", ctypes.c_size_t),
        ("fold_halo", ctypes.c_size_t),
        ("d_status", ctypes.c_void_p),
        ("trim", ctypes.c_size_t),
    ]


class DeviceOptsKrum(DeviceOpts):
    """struct fltee_device_opts_krum: the options of an OPT_KRUM call, DeviceOpts with Multi-Krum's
    two counts behind it (passed wherever a DeviceOpts pointer is taken; read under the flag)."""
    _fields_ = [
        ("krum_f", ctypes.c_size_t),
        ("krum_m", ctypes.c_size_t),
    ]


class DeviceOptsGmed(DeviceOpts):
    """struct fltee_device_opts_gmed: the options of an OPT_GMED call, DeviceOpts with the iteration
    count and the smoothing floor behind it (passed wherever a DeviceOpts pointer is taken; read
    under the flag)."""
    _fields_ = [
        ("gmed_iters", ctypes.c_size_t),
        ("gmed_nu", ctypes.c_double),
    ]


# every symbol declared in include/fltee_agg.h, with its ctypes signature
_P, _S, _U32, _U64, _F, _U8 = (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32,
                               ctypes.c_uint64, ctypes.c_float, ctypes.c_uint8)
SIGNATURES = {
    "fltee_device_init": (_U32, [ctypes.c_int, _P]),
    "fltee_device_fini": (_U32, [_U64]),
    "ecall_fl_init": (_U32, [_U64, _P, _U32, _P, _S, _S, _S, _F, _F, _F, _F, _U32, _U8, _U8]),
    "ecall_start_round": (_U32, [_U64, _P, _U32, _U32, _S, _P]),
    "ecall_secure_aggregation": (_U32, [_U64, _P, _U32, _U32, _P, _S, _P, _S, _S, _S, _U32, _P, _P]),
    "ecall_client_size_optimized_secure_aggregation":
        (_U32, [_U64, _P, _U32, _U32, _S, _P, _S, _P, _S, _S, _U32, _P, _P]),
    "fltee_aggregate_device": (_U32, [_U32, _P, _S, _S, _S, _P, ctypes.POINTER(DeviceOpts), _P]),
    "fltee_workspace_bytes": (_S, [_U32, _S, _S, _S, ctypes.POINTER(DeviceOpts)]),
    "fltee_reserve": (_U32, [_U32, _S, _S, _S, ctypes.POINTER(DeviceOpts)]),
    "fltee_decrypt_device": (_U32, [_P, _S, _P, _S, _P, _P]),
    "fltee_decrypt_auth_device": (_U32, [_P, _S, _P, _S, _P, _P, _S, _P, _P, _P]),
    "fltee_encrypt_auth_device": (_U32, [_P, _S, _P, _S, _P, _P, _S, _P, _P]),
    "fltee_debug_gcm_tag_host": (_U32, [_U32, _P, _P, _S, _P, _S, _P]),
    "fltee_gcm_segments": (_S, [_S, _S]),
    "fltee_ghash_window_device": (_U32, [_P, _S, _P, _S, _S, _S, _S, _P, _S, ctypes.c_int, _P, _P]),
    "fltee_ghash_merge_device": (_U32, [_P, _P, _S, _S, _P]),
    "fltee_gcm_finish_device": (_U32, [_P, _S, _P, _S, _P, _S, _P, _P, _P]),
    "fltee_decrypt_slice_auth_device": (_U32, [_P, _S, _P, _S, _S, _S, _P, _P, _P]),
    "fltee_debug_ghash_window_host": (_U32, [_U32, _P, _S, ctypes.c_int, _P, _S, _S, _S, _P]),
    "fltee_packed_slice_bytes": (_S, [_S]),
    "fltee_upload_is_packed": (ctypes.c_int, [ctypes.c_int, _S, _S, _S]),
    "fltee_set_upload_packed": (None, [ctypes.c_int]),
    "fltee_unpack_dense_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_client_pack_dense_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_trim_count": (_S, [_S, _U32]),
    "fltee_set_dense_trim": (None, [_U32]),
    "fltee_set_dense_trim_select": (None, [ctypes.c_int]),
    "fltee_krum_select_device": (_U32, [_P, _S, _S, ctypes.POINTER(DeviceOpts), _P, _P, _P]),
    "fltee_krum_gram_ranges_device": (_U32, [_P, ctypes.c_int, _S, _S, _U32, _P]),
    "fltee_set_dense_krum": (None, [_U32, _U32]),
    "fltee_gmed_weights_device": (_U32, [_P, _S, _S, ctypes.POINTER(DeviceOpts), _P, _P, _P]),
    "fltee_set_dense_gmed": (None, [_U32, ctypes.c_double]),
    "fltee_bf16_slice_bytes": (_S, [_S]),
    "fltee_upload_is_bf16": (ctypes.c_int, [ctypes.c_int, _S, _S, _S]),
    "fltee_set_upload_bf16": (None, [ctypes.c_int]),
    "fltee_unpack_bf16_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_client_pack_bf16_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_fp8_slice_bytes": (_S, [_S]),
    "fltee_upload_is_fp8": (ctypes.c_int, [ctypes.c_int, _S, _S, _S]),
    "fltee_set_upload_fp8": (None, [ctypes.c_int]),
    "fltee_unpack_fp8_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_client_pack_fp8_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_set_upload_aead": (None, [ctypes.c_int]),
    "fltee_set_upload_aead_policy": (None, [ctypes.c_int, _S]),
    "fltee_auth_report": (_U32, [_U64, _U32, _P, _P, _S, _P]),
    "fltee_gather_clients_device": (_U32, [_P, _S, _S, _P, _S, _P, _P]),
    "fltee_device_status": (_U32, [_P, _P]),
    "fltee_sum_rows_device": (_U32, [_P, _S, _S, _F, _P, _P]),
    "fltee_dp_noise_device": (_U32, [_P, _S, _F, _F, _S, _U64, _P]),
    "fltee_bitonic_device": (_U32, [_P, _S, _U32, _U32, _P]),
    "fltee_stable_sort_device": (_U32, [_P, _S, _P]),
    "fltee_fold_device": (_U32, [_P, _P, _S, _S, _S, _P, _P]),
    "fltee_laplace_r_device": (_U32, [_S, _S, _S, _U64, _P, _P, _P]),
    "fltee_client_topk_device": (_U32, [_P, _S, _S, _S, _P, _P]),
    "fltee_client_serialize_dense_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_client_clip_device": (_U32, [_P, _S, _S, _F, _P]),
    "fltee_encrypt_device": (_U32, [_P, _S, _P, _S, _P, _P]),
    "fltee_advanced_init_range_device": (_U32, [_P, _S, _S, _S, _S, _P, _P]),
    "fltee_bitonic_range_sort_device": (_U32, [_P, _S, _S, _U32, _U32, _P]),
    "fltee_bitonic_range_sort_padded_device": (_U32, [_P, _S, _S, _S, _U32, _U32, _P]),
    "fltee_bitonic_range_merge_device": (_U32, [_P, _S, _S, _U32, _U32, _U32, _P]),
    "fltee_bitonic_range_exchange_device": (_U32, [_P, _P, _S, _S, _S, _U32, _U32, _U32, _P]),
    "fltee_bitonic_range_steps_device": (_U32, [_P, _S, _S, _U32, _U32, _U32, _U32, _U32, _P]),
    "fltee_stable_init_range_device": (_U32, [_P, _S, _S, _S, _S, _P, _P]),
    "fltee_stable_range_sort_device": (_U32, [_P, _S, _S, _S, _P]),
    "fltee_stable_range_exchange_device": (_U32, [_P, _P, _S, _S, _S, _U32, _P]),
    "fltee_stable_range_merge_device": (_U32, [_P, _S, _S, _U32, _P]),
    "fltee_stable_range_strip_device": (_U32, [_P, _S, _P, _P]),
    "fltee_fold_context": (_S, [_S]),
    "fltee_fold_side_bytes": (_S, [_S, _S]),
    "fltee_fold_range_device": (_U32, [_P, _P, _S, _S, _S, ctypes.c_int64, _S, _S, _P, _P]),
    "fltee_fold_range_total_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_fold_range_patch_device": (_U32, [_P, _S, _S, ctypes.c_int64, _S, _S, _P, _P, _S, _P]),
    "fltee_compact_range_device": (_U32, [_P, _S, _S, _P, _P, _F, _P, _P]),
    "fltee_nips19_build_range_device": (_U32, [_P, _S, _P, _S, _S, _S, _S, _P, _P]),
    "fltee_safe_aggregate_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_select_device": (_U32, [_P, _S, _S, _P, _S, _P, _P]),
    "fltee_ordered_list_device": (_U32, [_P, _S, _S, _F, _P, _P]),
    "fltee_debug_sort_records_device": (_U32, [_P, _S, _S, _P, _P]),
    "fltee_debug_set_seed": (None, [_U64]),
    "fltee_set_path_oram_tree": (None, [ctypes.c_int]),
    "fltee_set_advanced_exact_runs": (None, [ctypes.c_int]),
    "fltee_set_bubble_ecall": (None, [ctypes.c_int]),
    "fltee_version": (ctypes.c_char_p, []),
    "fltee_device_init_multi": (_U32, [_P, ctypes.c_int, _P]),
    "fltee_device_count": (ctypes.c_int, [_U64]),
}
EXTRA_SIGNATURES = {  # test hooks not in the public header
    "fltee_debug_aes_block": (None, [_P, _P, _P]),
    "fltee_debug_gf128_mul": (None, [_P, _P, _P]),
    "fltee_debug_gcm_subkeys": (ctypes.c_int, [_U32, _P, _P, ctypes.c_int]),
    "fltee_debug_gcm_segment_blocks": (_S, []),
    "fltee_debug_set_dense_variant": (None, [ctypes.c_int]),
    "fltee_debug_set_oram_bucket": (None, [ctypes.c_int]),
    "fltee_debug_set_aes_variant": (None, [ctypes.c_int]),
    "fltee_debug_read_floor": (ctypes.c_int, [_P, _S, _P, ctypes.c_uint, _P]),
    "fltee_debug_network_plan": (_S, [_U32, _U32, _U32, ctypes.c_int, _P, _S]),
    "fltee_debug_pad_units": (None, [_U32] * 8 + [_P]),
    "fltee_debug_set_advanced_compaction": (None, [ctypes.c_int]),
    "fltee_debug_set_compact_variant": (None, [ctypes.c_int]),
    "fltee_debug_set_fused_init": (None, [ctypes.c_int]),
    "fltee_debug_set_nips19_fused_select": (None, [ctypes.c_int]),
    "fltee_debug_net_stats": (None, [_P, _P, ctypes.c_int]),
    "fltee_debug_net_timing": (None, [ctypes.c_int, _P]),
    "fltee_debug_session_round_keys": (ctypes.c_int, [_P, _S, _P, ctypes.c_int]),
    "fltee_debug_net_log": (_S, [_S, ctypes.c_char_p, _S, _P, _P]),
    "fltee_debug_set_fold_compact": (None, [ctypes.c_int]),
    "fltee_debug_fold_geometry": (None, [_S, _S, _S, _S, _P]),
    "fltee_debug_plan": (_U32, [_U32, _S, _S, _S, ctypes.POINTER(DeviceOpts), _P]),
    "fltee_debug_scratch_grown": (_U32, []),
    "fltee_debug_krum_geometry": (None, [_S, _S, _P]),
    "fltee_debug_scratch_release": (None, []),
    "fltee_debug_set_pad_skip": (None, [ctypes.c_int]),
    "fltee_debug_set_radix_order": (None, [ctypes.c_int]),
    "fltee_debug_set_swizzle": (None, [ctypes.c_int]),
    "fltee_debug_sort_fused": (_U32, [_U32, _P, _S, _P, _S, _P, _S, _S,
                                       _U32, _P]),
}

_lib = None


def lib():
    """Load the HIP library (raises if it was not built: no fallback path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `make -C {PKG_ROOT}` "
                "(the aggregation path has no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        ab = bool(os.environ.get("FLTEE_LIB"))  # an A/B build of an older source may lack a hook
        for name, (res, args) in {**SIGNATURES, **EXTRA_SIGNATURES}.items():
            if ab and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib

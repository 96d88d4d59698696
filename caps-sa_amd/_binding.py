"""ctypes binding of the C ABI declared in include/caps_sa_hip.h.

``CapsLib(path, prefix)`` binds one shared library.  The product package binds
libcaps_sa_hip.so (prefix ``caps_sa_hip_``); tests bind the host emulation of the same
sources (tests/emul/libcaps_sa_emul.so, prefix ``caps_sa_emul_``) through this class too.
"""
from __future__ import annotations

import ctypes
import weakref

import numpy as np

_u64, _vp, _ci = ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int


class Stats(ctypes.Structure):
    """caps_sa_stats (include/caps_sa_hip.h)."""
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("idx_bytes", ctypes.c_uint32),
        ("p_eff", ctypes.c_uint32),
        ("ppp", ctypes.c_uint32),
        ("bits_per_char", ctypes.c_uint32),
        ("merge_passes_phase1", ctypes.c_uint32),
        ("merge_passes_phase2", ctypes.c_uint32),
        ("merge_passes_samples", ctypes.c_uint32),
        ("long_runs", ctypes.c_uint32),
        ("max_partition", ctypes.c_uint64),
        ("workspace_bytes", ctypes.c_uint64),
        ("ms_total", ctypes.c_double),
        ("ms_pack", ctypes.c_double),
        ("ms_sort_subarrays", ctypes.c_double),
        ("ms_select_pivots", ctypes.c_double),
        ("ms_locate_pivots", ctypes.c_double),
        ("ms_partition", ctypes.c_double),
        ("ms_merge_partitions", ctypes.c_double),
        ("ms_boundary_lcp", ctypes.c_double),
        ("ms_output", ctypes.c_double),
        ("ms_h2d", ctypes.c_double),
        ("ms_d2h", ctypes.c_double),
        ("merge_pass_ms", ctypes.c_double),
        ("merge_pass_launches", ctypes.c_uint64),
        ("merge_pass_elems", ctypes.c_uint64),
        ("tile_sort_ms", ctypes.c_double),
        ("tile_sort_launches", ctypes.c_uint64),
        ("tile_sort_elems", ctypes.c_uint64),
        ("bucket_scatter_ms", ctypes.c_double),
        ("bucket_scatter_launches", ctypes.c_uint64),
        ("bucket_scatter_elems", ctypes.c_uint64),
        ("bucket_count_ms", ctypes.c_double),
        ("collate_ms", ctypes.c_double),
        ("slot_splits", ctypes.c_uint32),
        ("slot_splits_redone", ctypes.c_uint32),
        ("path_direct", ctypes.c_uint32),
        ("path_fallback", ctypes.c_uint32),
        ("direct_groups", ctypes.c_uint32),
        ("direct_quantile", ctypes.c_uint32),
        ("direct_max_group", ctypes.c_uint64),
        ("level_a_ms", ctypes.c_double),
        ("direct_key_bits", ctypes.c_uint32),
        ("run_buckets", ctypes.c_uint32),
        ("result_waves", ctypes.c_uint32),
        ("n_devices", ctypes.c_uint32),
        ("ms_upload_max", ctypes.c_double),
        ("ms_upload_min", ctypes.c_double),
        ("ms_device_build_max", ctypes.c_double),
        ("ms_device_build_min", ctypes.c_double),
        ("ms_download_max", ctypes.c_double),
        ("ms_download_min", ctypes.c_double),
        ("tie_groups_deferred", ctypes.c_uint64),
        ("tie_elems_deferred", ctypes.c_uint64),
        ("tie_levels", ctypes.c_uint32),
        ("lcp_bytes_on_link", ctypes.c_uint32),
        ("finish_ms", ctypes.c_double),
        ("run_bucket_ms", ctypes.c_double),
        ("msd_ms", ctypes.c_double),
        ("knot_slot_splits", ctypes.c_uint32),
        ("knot_slot_splits_redone", ctypes.c_uint32),
        ("spill_entries", ctypes.c_uint64),
        ("direct_records", ctypes.c_uint32),
        ("tile_chain", ctypes.c_uint32),
        ("scatter_issue", ctypes.c_uint32),
        ("slot_keys", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


class ShardInfo(ctypes.Structure):
    """caps_sa_shard_info (include/caps_sa_hip.h)."""
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("p", ctypes.c_uint32), ("ppp", ctypes.c_uint32), ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32),
        ("g0", ctypes.c_uint32), ("g1", ctypes.c_uint32),
        ("bits_per_char", ctypes.c_uint32), ("idx_bytes", ctypes.c_uint32),
        ("part_lo", ctypes.c_uint32), ("part_hi", ctypes.c_uint32),
        ("local_elems", ctypes.c_uint64),
        ("m_local", ctypes.c_uint64), ("m_total", ctypes.c_uint64),
        ("recv_total", ctypes.c_uint64),
        ("slice_off", ctypes.c_uint64),
        ("capacity", ctypes.c_uint64),
        ("ms_phase1", ctypes.c_double), ("ms_pivots", ctypes.c_double), ("ms_collate", ctypes.c_double),
        ("ms_phase2", ctypes.c_double),
        ("direct_fallback", ctypes.c_uint32), ("direct_groups", ctypes.c_uint32), ("direct_sub", ctypes.c_uint32),
        ("n_streams", ctypes.c_uint32),
        ("stream_cap", ctypes.c_uint64), ("send_capacity", ctypes.c_uint64),
        ("ms_scatter", ctypes.c_double), ("ms_sort", ctypes.c_double),
        ("ms_level_a", ctypes.c_double), ("ms_level_b", ctypes.c_double), ("ms_tile_sort", ctypes.c_double),
        ("ms_merge_passes", ctypes.c_double),
        ("level_a_elems", ctypes.c_uint64),
        ("slot_splits", ctypes.c_uint32), ("slot_splits_redone", ctypes.c_uint32),
        ("key_bytes", ctypes.c_uint32), ("exchange", ctypes.c_uint32),
        ("direct_quantile", ctypes.c_uint32), ("run_buckets", ctypes.c_uint32),
        ("tie_groups_deferred", ctypes.c_uint64), ("tie_levels", ctypes.c_uint32), ("reserved_", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


SHARD_EXPORTS = ["shard_create", "shard_destroy", "shard_info", "shard_phase1", "shard_pivots", "shard_collate",
                 "shard_phase2", "shard_last_sa", "shard_fix_first_lcp", "shard_scatter", "shard_plan", "shard_sort",
                 "shard_phase1_arrays", "shard_set_key_bits"]

EXPORTS = ["device_count", "last_error", "version", "stats_bytes", "shard_info_bytes", "workspace_bytes", "workspace_bytes_ex", "release_cache", "host_alloc", "host_free", "gen_rand_seq",
           "inverse_bwt_workspace_bytes", "fm_index_bytes", "fm_from_bwt_workspace_bytes", "fm_count", "fm_locate", "fm_count_device", "fm_locate_device",
           "fm_index_bytes_ex", "fm_add_text_samples", "fm_add_text_samples_device", "fm_extract_workspace_bytes", "fm_extract", "fm_extract_device",
           "fm_match", "fm_match_device", "fm_mems_workspace_bytes", "fm_mems", "fm_mems_device", "fm_wide_index_bytes",
           "fm_wide_workspace_bytes", "kmer_workspace_bytes", "cross_workspace_bytes", "coll_workspace_bytes", "lpf_workspace_bytes", "lz77_workspace_bytes", "lce_index_bytes",
           "lce_range_min", "lce_range_min_device", "lce", "lce_device"] + SHARD_EXPORTS + [
    f"{name}_{sfx}"
    for sfx in ("u32", "u64")
    for name in ("build", "build_multi", "build_device", "verify_device", "verify_slice_device", "sort_suffixes", "sort_segments", "merge",
                 "upper_bound", "lcp", "build_bwt", "bwt_device", "inverse_bwt", "inverse_bwt_device", "fm_build", "fm_build_device",
                 "fm_build_from_bwt", "fm_build_from_bwt_device", "fm_build_wide", "fm_build_wide_device",
                 "kmers", "kmers_device", "kmer_spectrum", "kmer_spectrum_device", "kmer_census", "kmer_census_device",
                 "lpf", "lpf_device", "lz77", "lz77_device", "isa", "isa_device", "lce_build", "lce_build_device",
                 "cross_mums", "cross_mums_device", "cross_mems", "cross_mems_device",
                 "coll_kmers", "coll_kmers_device", "coll_sharing", "coll_sharing_device")
]


# a MEM record of fm_mems (include/caps_sa_hip.h "FM-index: matching statistics"): 32 bytes, little-endian
MEM_DTYPE = np.dtype([("pattern", "<u8"), ("start", "<u4"), ("length", "<u4"), ("first", "<u8"), ("count", "<u8")])

# a record of kmers (include/caps_sa_hip.h "k-mers from SA and LCP"): 24 bytes, little-endian
KMER_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("pos", "<u8")])

# a record of cross_mums / cross_mems (include/caps_sa_hip.h "MUMs and MEMs between two texts"): 24 bytes, little-endian
CROSS_DTYPE = np.dtype([("a", "<u8"), ("b", "<u8"), ("len", "<u8")])
CROSS_MAX_OCC = 64

# a record of coll_kmers (include/caps_sa_hip.h "k-mers across a collection"): 32 bytes, little-endian
COLL_DTYPE = np.dtype([("first", "<u8"), ("count", "<u8"), ("occ", "<u8"), ("docs", "<u8")])
COLL_MAX_DOCS = 64

# a phrase of lz77 (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP"): 24 bytes, little-endian; src = LZ_LITERAL: one byte
LZ_DTYPE = np.dtype([("pos", "<u8"), ("len", "<u8"), ("src", "<u8")])
LZ_LITERAL = 0xFFFFFFFFFFFFFFFF


class CapsSaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"caps_sa error {code}: {msg}")
        self.code = code


def _sfx(idx_bits: int):
    return {32: ("u32", np.uint32), 64: ("u64", np.uint64)}[idx_bits]


class CapsLib:
    def __init__(self, path: str, prefix: str = "caps_sa_hip_"):
        self.path = path
        self.prefix = prefix
        self.dll = ctypes.CDLL(path)
        f = self._f
        f("device_count").restype = _ci
        f("device_count").argtypes = []
        f("last_error").restype = ctypes.c_char_p
        f("version").restype = ctypes.c_char_p
        # the structs grow at their end from release to release and the library writes all of them: a mirror of another size
        # would be overrun (or read short) -- refuse to work with it
        for name, mirror in (("stats_bytes", Stats), ("shard_info_bytes", ShardInfo)):
            f(name).restype = ctypes.c_uint32
            f(name).argtypes = []
            if f(name)() != ctypes.sizeof(mirror):
                raise CapsSaError(-1, f"{path}: its {name} = {f(name)()}, this binding's mirror has {ctypes.sizeof(mirror)} "
                                      "(library and _binding.py are of different versions)")
        f("workspace_bytes").restype = _ci
        f("workspace_bytes").argtypes = [_u64, _u64, _ci, ctypes.POINTER(_u64)]
        f("workspace_bytes_ex").restype = _ci
        f("workspace_bytes_ex").argtypes = [_u64, _u64, _ci, _ci, ctypes.POINTER(_u64)]
        f("release_cache").restype = None
        f("release_cache").argtypes = []
        f("host_alloc").restype = _vp
        f("host_alloc").argtypes = [_u64]
        f("host_free").restype = None
        f("host_free").argtypes = [_vp]
        f("gen_rand_seq").restype = _ci
        f("gen_rand_seq").argtypes = [ctypes.c_uint32, _u64, _vp]
        f("inverse_bwt_workspace_bytes").restype = _ci
        f("inverse_bwt_workspace_bytes").argtypes = [_u64, _ci, ctypes.POINTER(_u64)]
        f("fm_index_bytes").restype = _ci
        f("fm_index_bytes").argtypes = [_u64, ctypes.c_uint32, _ci, ctypes.POINTER(_u64)]
        f("fm_count").restype = _ci
        f("fm_count").argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _vp, _ci]
        f("fm_locate").restype = _ci
        f("fm_locate").argtypes = [_vp, _u64, _vp, _vp, _vp, _u64, _vp, _ci]
        f("fm_count_device").restype = _ci
        f("fm_count_device").argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _vp, _vp]
        f("fm_locate_device").restype = _ci
        f("fm_locate_device").argtypes = [_vp, _u64, _vp, _vp, _vp, _u64, _vp, _vp]
        f("fm_index_bytes_ex").restype = _ci
        f("fm_index_bytes_ex").argtypes = [_u64, ctypes.c_uint32, ctypes.c_uint32, _ci, ctypes.POINTER(_u64)]
        f("fm_add_text_samples").restype = _ci
        f("fm_add_text_samples").argtypes = [_vp, _u64, ctypes.c_uint32, _ci]
        f("fm_add_text_samples_device").restype = _ci
        f("fm_add_text_samples_device").argtypes = [_vp, _u64, ctypes.c_uint32, _vp]
        f("fm_extract_workspace_bytes").restype = _ci
        f("fm_extract_workspace_bytes").argtypes = [_u64, ctypes.POINTER(_u64)]
        f("fm_extract").restype = _ci
        f("fm_extract").argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _ci]
        f("fm_extract_device").restype = _ci
        f("fm_extract_device").argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _vp, _u64, _vp]
        f("fm_match").restype = _ci
        f("fm_match").argtypes = [_vp, _u64, _vp, _vp, _u64, ctypes.c_uint32, _vp, _vp, _vp, _ci]
        f("fm_match_device").restype = _ci
        f("fm_match_device").argtypes = [_vp, _u64, _vp, _vp, _u64, ctypes.c_uint32, _vp, _vp, _vp, _vp]
        f("fm_mems_workspace_bytes").restype = _ci
        f("fm_mems_workspace_bytes").argtypes = [_u64, _u64, ctypes.POINTER(_u64)]
        f("fm_mems").restype = _ci
        f("fm_mems").argtypes = [_vp, _u64, _vp, _vp, _u64, ctypes.c_uint32, _vp, _vp, _u64, _ci]
        f("fm_mems_device").restype = _ci
        f("fm_mems_device").argtypes = [_vp, _u64, _vp, _vp, _u64, ctypes.c_uint32, _vp, _vp, _u64, _vp, _u64, _vp]
        f("fm_from_bwt_workspace_bytes").restype = _ci
        f("fm_from_bwt_workspace_bytes").argtypes = [_u64, ctypes.c_uint32, _ci, ctypes.POINTER(_u64)]
        f("fm_wide_index_bytes").restype = _ci
        f("fm_wide_index_bytes").argtypes = [_u64, ctypes.c_uint32, ctypes.c_uint32, _ci, ctypes.POINTER(_u64)]
        f("fm_wide_workspace_bytes").restype = _ci
        f("fm_wide_workspace_bytes").argtypes = [_u64, _ci, ctypes.POINTER(_u64)]
        f("kmer_workspace_bytes").restype = _ci
        f("kmer_workspace_bytes").argtypes = [_u64, _ci, ctypes.POINTER(_u64)]
        f("cross_workspace_bytes").restype = _ci
        f("cross_workspace_bytes").argtypes = [_u64, _ci, ctypes.POINTER(_u64)]
        f("coll_workspace_bytes").restype = _ci
        f("coll_workspace_bytes").argtypes = [_u64, _ci, ctypes.POINTER(_u64)]
        for name in ("lpf_workspace_bytes", "lz77_workspace_bytes"):
            f(name).restype = _ci
            f(name).argtypes = [_u64, _ci, ctypes.POINTER(_u64)]
        f("lce_index_bytes").restype = _ci
        f("lce_index_bytes").argtypes = [_u64, _ci, ctypes.POINTER(_u64)]
        f("lce_range_min").restype = _ci
        f("lce_range_min").argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _ci]
        f("lce_range_min_device").restype = _ci
        f("lce_range_min_device").argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _vp]
        f("lce").restype = _ci
        f("lce").argtypes = [_vp, _u64, _vp, _vp, _u64, _u64, _vp, _ci]
        f("lce_device").restype = _ci
        f("lce_device").argtypes = [_vp, _u64, _vp, _vp, _u64, _u64, _vp, _vp]
        for sfx in ("u32", "u64"):
            f(f"isa_{sfx}").restype = _ci
            f(f"isa_{sfx}").argtypes = [_vp, _u64, _vp, _ci]
            f(f"isa_device_{sfx}").restype = _ci
            f(f"isa_device_{sfx}").argtypes = [_vp, _u64, _vp, _vp]
            f(f"lce_build_{sfx}").restype = _ci
            f(f"lce_build_{sfx}").argtypes = [_vp, _vp, _u64, _vp, _u64, _ci]
            f(f"lce_build_device_{sfx}").restype = _ci
            f(f"lce_build_device_{sfx}").argtypes = [_vp, _vp, _u64, _vp, _u64, _vp]
            f(f"lpf_{sfx}").restype = _ci
            f(f"lpf_{sfx}").argtypes = [_vp, _vp, _u64, _vp, _vp, _ci]
            f(f"lpf_device_{sfx}").restype = _ci
            f(f"lpf_device_{sfx}").argtypes = [_vp, _vp, _u64, _vp, _vp, _vp, _u64, _vp]
            f(f"lz77_{sfx}").restype = _ci
            f(f"lz77_{sfx}").argtypes = [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u64), _ci]
            f(f"lz77_device_{sfx}").restype = _ci
            f(f"lz77_device_{sfx}").argtypes = [_vp, _vp, _u64, _vp, _u64, ctypes.POINTER(_u64), _vp, _u64, _vp]
            f(f"cross_mums_{sfx}").restype = _ci
            f(f"cross_mums_{sfx}").argtypes = [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _ci]
            f(f"cross_mems_{sfx}").restype = _ci
            f(f"cross_mems_{sfx}").argtypes = [_vp, _vp, _vp, _u64, _u64, _u64, ctypes.c_uint32, _vp, _u64, _vp, _ci]
            f(f"cross_mums_device_{sfx}").restype = _ci
            f(f"cross_mums_device_{sfx}").argtypes = [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp]
            f(f"cross_mems_device_{sfx}").restype = _ci
            f(f"cross_mems_device_{sfx}").argtypes = [_vp, _vp, _vp, _u64, _u64, _u64, ctypes.c_uint32, _vp, _u64, _vp, _vp, _u64, _vp]
            _docs = [_vp, _vp, ctypes.c_uint32]
            f(f"coll_kmers_{sfx}").restype = _ci
            f(f"coll_kmers_{sfx}").argtypes = [_vp, _vp, _u64, _u64] + _docs + [_u64, _u64, _u64, _u64, _vp, _u64, _vp, _ci]
            f(f"coll_kmers_device_{sfx}").restype = _ci
            f(f"coll_kmers_device_{sfx}").argtypes = [_vp, _vp, _u64, _u64] + _docs + [_u64, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _u64, _vp]
            f(f"coll_sharing_{sfx}").restype = _ci
            f(f"coll_sharing_{sfx}").argtypes = [_vp, _vp, _u64, _u64] + _docs + [_vp, _vp, _ci]
            f(f"coll_sharing_device_{sfx}").restype = _ci
            f(f"coll_sharing_device_{sfx}").argtypes = [_vp, _vp, _u64, _u64] + _docs + [_vp, _vp, _vp, _u64, _vp]
            f(f"kmers_{sfx}").restype = _ci
            f(f"kmers_{sfx}").argtypes = [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _u64, ctypes.POINTER(_u64), _ci]
            f(f"kmers_device_{sfx}").restype = _ci
            f(f"kmers_device_{sfx}").argtypes = [_vp, _vp, _u64, _u64, _u64, _u64, _vp, _u64, ctypes.POINTER(_u64), _vp, _u64, _vp]
            f(f"kmer_spectrum_{sfx}").restype = _ci
            f(f"kmer_spectrum_{sfx}").argtypes = [_vp, _vp, _u64, _u64, ctypes.c_uint32, _vp, _ci]
            f(f"kmer_spectrum_device_{sfx}").restype = _ci
            f(f"kmer_spectrum_device_{sfx}").argtypes = [_vp, _vp, _u64, _u64, ctypes.c_uint32, _vp, _vp, _u64, _vp]
            f(f"kmer_census_{sfx}").restype = _ci
            f(f"kmer_census_{sfx}").argtypes = [_vp, _vp, _u64, ctypes.c_uint32, _vp, _vp, _ci]
            f(f"kmer_census_device_{sfx}").restype = _ci
            f(f"kmer_census_device_{sfx}").argtypes = [_vp, _vp, _u64, ctypes.c_uint32, _vp, _vp, _vp, _u64, _vp]
            f(f"fm_build_wide_{sfx}").restype = _ci
            f(f"fm_build_wide_{sfx}").argtypes = [_vp, _u64, _u64, _vp, ctypes.c_uint32, _vp, _u64, _ci]
            f(f"fm_build_wide_device_{sfx}").restype = _ci
            f(f"fm_build_wide_device_{sfx}").argtypes = [_vp, _u64, _u64, _vp, ctypes.c_uint32, _vp, _u64, _vp, _u64, _vp]
            f(f"fm_build_from_bwt_{sfx}").restype = _ci
            f(f"fm_build_from_bwt_{sfx}").argtypes = [_vp, _u64, _u64, ctypes.c_uint32, _vp, _u64, _ci]
            f(f"fm_build_from_bwt_device_{sfx}").restype = _ci
            f(f"fm_build_from_bwt_device_{sfx}").argtypes = [_vp, _u64, _u64, ctypes.c_uint32, _vp, _u64, _vp, _u64, _vp]
            f(f"fm_build_{sfx}").restype = _ci
            f(f"fm_build_{sfx}").argtypes = [_vp, _u64, _u64, _vp, ctypes.c_uint32, _vp, _u64, _ci]
            f(f"fm_build_device_{sfx}").restype = _ci
            f(f"fm_build_device_{sfx}").argtypes = [_vp, _u64, _u64, _vp, ctypes.c_uint32, _vp, _u64, _vp]
            f(f"build_{sfx}").restype = _ci
            f(f"build_{sfx}").argtypes = [_vp, _u64, _u64, _u64, _vp, _vp, _ci, ctypes.POINTER(Stats)]
            f(f"build_multi_{sfx}").restype = _ci
            f(f"build_multi_{sfx}").argtypes = [_vp, _u64, _u64, _u64, _vp, _vp, _vp, _ci, ctypes.POINTER(Stats)]
            f(f"build_device_{sfx}").restype = _ci
            f(f"build_device_{sfx}").argtypes = [_vp, _u64, _u64, _u64, _vp, _vp, _vp, _u64, _vp, ctypes.POINTER(Stats)]
            f(f"build_bwt_{sfx}").restype = _ci
            f(f"build_bwt_{sfx}").argtypes = [_vp, _u64, _u64, _u64, _vp, _vp, _vp, ctypes.POINTER(_u64), _ci, ctypes.POINTER(Stats)]
            f(f"bwt_device_{sfx}").restype = _ci
            f(f"bwt_device_{sfx}").argtypes = [_vp, _u64, _vp, _u64, _u64, _vp, _vp, ctypes.POINTER(_u64)]
            f(f"inverse_bwt_{sfx}").restype = _ci
            f(f"inverse_bwt_{sfx}").argtypes = [_vp, _u64, _u64, _vp, _ci]
            f(f"inverse_bwt_device_{sfx}").restype = _ci
            f(f"inverse_bwt_device_{sfx}").argtypes = [_vp, _u64, _u64, _vp, _vp, _u64, _vp]
            f(f"verify_device_{sfx}").restype = _ci
            f(f"verify_device_{sfx}").argtypes = [_vp, _u64, _vp, _vp, _vp, ctypes.POINTER(_u64)]
            f(f"verify_slice_device_{sfx}").restype = _ci
            f(f"verify_slice_device_{sfx}").argtypes = [_vp, _u64, _vp, _vp, _u64, _ci, _vp, ctypes.POINTER(_u64)]
            f(f"sort_suffixes_{sfx}").restype = _ci
            f(f"sort_suffixes_{sfx}").argtypes = [_vp, _u64, _vp, _u64, _vp, _vp, _ci]
            f(f"sort_segments_{sfx}").restype = _ci
            f(f"sort_segments_{sfx}").argtypes = [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _ci]
            f(f"merge_{sfx}").restype = _ci
            f(f"merge_{sfx}").argtypes = [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _ci]
            f(f"upper_bound_{sfx}").restype = _ci
            f(f"upper_bound_{sfx}").argtypes = [_vp, _u64, _vp, _u64, _vp, _u64, _vp, _ci]
            f(f"lcp_{sfx}").restype = _ci
            f(f"lcp_{sfx}").argtypes = [_vp, _u64, _vp, _vp, _u64, _vp, _ci]

        f("shard_create").restype = _ci
        f("shard_create").argtypes = [_vp, _u64, _u64, _ci, _ci, _ci, _vp, ctypes.POINTER(_vp)]
        f("shard_destroy").restype = None
        f("shard_destroy").argtypes = [_vp]
        f("shard_info").restype = _ci
        f("shard_info").argtypes = [_vp, ctypes.POINTER(ShardInfo)]
        f("shard_phase1").restype = _ci
        f("shard_phase1").argtypes = [_vp, _vp, _vp]
        f("shard_pivots").restype = _ci
        f("shard_pivots").argtypes = [_vp, _vp, _vp, _vp]
        f("shard_collate").restype = _ci
        f("shard_collate").argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
        f("shard_phase2").restype = _ci
        f("shard_phase2").argtypes = [_vp, _vp, _vp, _vp, _vp]
        f("shard_scatter").restype = _ci
        f("shard_scatter").argtypes = [_vp, _vp, _vp, _vp]
        f("shard_plan").restype = _ci
        f("shard_plan").argtypes = [_vp, _vp, _vp, _vp]
        f("shard_sort").restype = _ci
        f("shard_sort").argtypes = [_vp, _vp, _vp, _vp, _vp]
        f("shard_set_key_bits").restype = _ci
        f("shard_set_key_bits").argtypes = [_vp, _ci]
        f("shard_phase1_arrays").restype = _ci
        f("shard_phase1_arrays").argtypes = [_vp, _vp, _vp, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]
        f("shard_last_sa").restype = _ci
        f("shard_last_sa").argtypes = [_vp, ctypes.POINTER(_u64)]
        f("shard_fix_first_lcp").restype = _ci
        f("shard_fix_first_lcp").argtypes = [_vp, _u64, _vp]

    def _f(self, name: str):
        return getattr(self.dll, self.prefix + name)

    def shard(self, dT_ptr: int, n: int, p: int, idx_bits: int, rank: int, world: int, stream: int = 0) -> "Shard":
        return Shard(self, dT_ptr, n, p, idx_bits, rank, world, stream)

    def _check(self, rc: int):
        if rc != 0:
            raise CapsSaError(rc, self._f("last_error")().decode(errors="replace"))

    # ------------------------------------------------------------------ queries
    def device_count(self) -> int:
        return self._f("device_count")()

    def version(self) -> str:
        return self._f("version")().decode()

    def workspace_bytes(self, n: int, p: int = 0, idx_bits: int = 32, bits_per_char: int = 8) -> int:
        """bits_per_char = 2: a text of at most 4 distinct bytes (anything behind the reference CLI) -- a smaller text arena."""
        out = _u64(0)
        self._check(self._f("workspace_bytes_ex")(n, p, idx_bits // 8, bits_per_char, ctypes.byref(out)))
        return out.value

    # ------------------------------------------------------------------ host-buffer build
    @staticmethod
    def _text(T) -> np.ndarray:
        if isinstance(T, (bytes, bytearray)):
            T = np.frombuffer(bytes(T), dtype=np.uint8)
        return np.ascontiguousarray(T, dtype=np.uint8)

    def release_cache(self) -> None:
        """Frees the device memory the host-buffer entry points keep between calls."""
        self._f("release_cache")()

    def gen_rand_seq(self, seed: int, n: int, out: np.ndarray | None = None) -> np.ndarray:
        """n letters of the reference's utils/gen_rand_seq.py stream (host; see include/caps_sa_hip.h)."""
        if out is None:
            out = np.empty(n, dtype=np.uint8)
        assert out.dtype == np.uint8 and out.size >= n and out.flags.c_contiguous
        self._check(self._f("gen_rand_seq")(seed, n, out.ctypes.data))
        return out[:n]

    def pinned_empty(self, count: int, dtype) -> np.ndarray:
        """numpy array over page-locked host memory (caps_sa_hip_host_alloc); freed with the array."""
        dtype = np.dtype(dtype)
        nbytes = max(1, count * dtype.itemsize)
        ptr = self._f("host_alloc")(nbytes)
        if not ptr:
            raise CapsSaError(-12, (self._f("last_error")() or b"host_alloc failed").decode())
        buf = (ctypes.c_char * nbytes).from_address(ptr)
        arr = np.frombuffer(buf, dtype=dtype, count=count)
        free = self._f("host_free")
        weakref.finalize(buf, free, ptr)
        return arr

    def build(self, T, p: int = 0, max_context: int = 0, idx_bits: int = 32, device: int = 0, pinned: bool = False):
        """construct() on host buffers -> (SA, LCP, stats dict).  pinned: SA / LCP in page-locked memory."""
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        SA = self.pinned_empty(T.size, dt) if pinned else np.empty(T.size, dtype=dt)
        LCP = self.pinned_empty(T.size, dt) if pinned else np.empty(T.size, dtype=dt)
        st = Stats()
        self._check(self._f(f"build_{sfx}")(T.ctypes.data, T.size, p, max_context, SA.ctypes.data, LCP.ctypes.data,
                                            device, ctypes.byref(st)))
        return SA, LCP, st.as_dict()

    def build_into(self, T, SA: np.ndarray, LCP: np.ndarray, p: int = 0, max_context: int = 0, idx_bits: int = 32, device: int = 0) -> dict:
        """construct() into caller-owned result arrays (e.g. pinned_empty ones, re-used between calls) -> stats dict."""
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        assert SA.dtype == dt and LCP.dtype == dt and SA.size >= T.size and LCP.size >= T.size
        st = Stats()
        self._check(self._f(f"build_{sfx}")(T.ctypes.data, T.size, p, max_context, SA.ctypes.data, LCP.ctypes.data,
                                            device, ctypes.byref(st)))
        return st.as_dict()

    def build_bwt(self, T, p: int = 0, max_context: int = 0, idx_bits: int = 32, device: int = 0, pinned: bool = False):
        """construct() plus the Burrows-Wheeler transform (include/caps_sa_hip.h) -> (SA, LCP, BWT, primary, stats dict).
        BWT[k] = T[(SA[k] + n - 1) mod n] (np.uint8); primary = the k with SA[k] == 0 (2**64 - 1 when n = 0)."""
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        SA = self.pinned_empty(T.size, dt) if pinned else np.empty(T.size, dtype=dt)
        LCP = self.pinned_empty(T.size, dt) if pinned else np.empty(T.size, dtype=dt)
        BWT = self.pinned_empty(T.size, np.uint8) if pinned else np.empty(T.size, dtype=np.uint8)
        primary = _u64(0)
        st = Stats()
        self._check(self._f(f"build_bwt_{sfx}")(T.ctypes.data, T.size, p, max_context, SA.ctypes.data, LCP.ctypes.data, BWT.ctypes.data,
                                                ctypes.byref(primary), device, ctypes.byref(st)))
        return SA, LCP, BWT, primary.value, st.as_dict()

    def build_multi(self, T, devices, p: int = 0, max_context: int = 0, idx_bits: int = 32, pinned: bool = False):
        """construct() on several GPUs from this process (caps_sa_hip_build_multi_*) -> (SA, LCP, stats dict)."""
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        SA = self.pinned_empty(T.size, dt) if pinned else np.empty(T.size, dtype=dt)
        LCP = self.pinned_empty(T.size, dt) if pinned else np.empty(T.size, dtype=dt)
        devs = (ctypes.c_int * len(devices))(*devices)
        st = Stats()
        self._check(self._f(f"build_multi_{sfx}")(T.ctypes.data, T.size, p, max_context, SA.ctypes.data, LCP.ctypes.data,
                                                  devs, len(devices), ctypes.byref(st)))
        return SA, LCP, st.as_dict()

    # ------------------------------------------------------------------ device-resident build
    def build_device(self, dT_ptr: int, n: int, dSA_ptr: int, dLCP_ptr: int, p: int = 0, max_context: int = 0,
                     idx_bits: int = 32, workspace_ptr: int = 0, workspace_bytes: int = 0, stream: int = 0) -> dict:
        sfx, _ = _sfx(idx_bits)
        st = Stats()
        self._check(self._f(f"build_device_{sfx}")(dT_ptr, n, p, max_context, dSA_ptr, dLCP_ptr, workspace_ptr or None,
                                                   workspace_bytes, stream or None, ctypes.byref(st)))
        return st.as_dict()

    def verify_device(self, dT_ptr: int, n: int, dSA_ptr: int, dLCP_ptr: int, idx_bits: int = 32, stream: int = 0) -> int:
        sfx, _ = _sfx(idx_bits)
        err = _u64(0)
        self._check(self._f(f"verify_device_{sfx}")(dT_ptr, n, dSA_ptr, dLCP_ptr, stream or None, ctypes.byref(err)))
        return err.value

    def verify_slice_device(self, dT_ptr: int, n: int, dSA_ptr: int, dLCP_ptr: int, cnt: int, is_head: bool, idx_bits: int = 32,
                            stream: int = 0) -> int:
        sfx, _ = _sfx(idx_bits)
        err = _u64(0)
        self._check(self._f(f"verify_slice_device_{sfx}")(dT_ptr, n, dSA_ptr, dLCP_ptr, cnt, 1 if is_head else 0, stream or None,
                                                          ctypes.byref(err)))
        return err.value

    def bwt_device(self, dT_ptr: int, n: int, dSA_ptr: int, first: int, cnt: int, dBWT_ptr: int, idx_bits: int = 32,
                   stream: int = 0) -> int:
        """BWT of the suffix-array slice at dSA_ptr (ranks first .. first + cnt) into dBWT_ptr (cnt bytes, device) -> primary
        (first + k for the k with SA == 0 in the slice, else 2**64 - 1)."""
        sfx, _ = _sfx(idx_bits)
        primary = _u64(0)
        self._check(self._f(f"bwt_device_{sfx}")(dT_ptr or None, n, dSA_ptr or None, first, cnt, dBWT_ptr or None, stream or None,
                                                 ctypes.byref(primary)))
        return primary.value

    def inverse_bwt(self, BWT, primary: int, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """T back from (BWT, primary) (include/caps_sa_hip.h caps_sa_hip_inverse_bwt_*) -> np.uint8 array of n bytes.  The index
        width follows n unless idx_bits is given.  Not the BWT of any text: CapsSaError with code -1."""
        B = self._text(BWT)
        n = int(B.size)
        sfx, _ = _sfx(idx_bits or (32 if n <= 0xFFFFFFFF else 64))
        T = np.empty(n, dtype=np.uint8)
        self._check(self._f(f"inverse_bwt_{sfx}")(B.ctypes.data if n else None, n, int(primary), T.ctypes.data if n else None, device))
        return T

    def inverse_bwt_workspace_bytes(self, n: int, idx_bits: int = 32) -> int:
        out = _u64(0)
        self._check(self._f("inverse_bwt_workspace_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def inverse_bwt_device(self, dBWT_ptr: int, n: int, primary: int, dT_ptr: int, dWS_ptr: int, ws_bytes: int, idx_bits: int = 32,
                           stream: int = 0) -> None:
        """T back from (BWT, primary) in device memory: dBWT_ptr (n bytes) -> dT_ptr (n bytes), workspace dWS_ptr of ws_bytes
        (inverse_bwt_workspace_bytes)."""
        sfx, _ = _sfx(idx_bits)
        self._check(self._f(f"inverse_bwt_device_{sfx}")(dBWT_ptr or None, n, int(primary), dT_ptr or None, dWS_ptr or None, ws_bytes,
                                                         stream or None))

    # ------------------------------------------------------------------ FM-index (include/caps_sa_hip.h "FM-index")
    def fm_index_bytes(self, n: int, sa_sample: int = 32, idx_bits: int = 32) -> int:
        """Bytes of the index of n symbols; sa_sample = 0: without SA samples (count only)."""
        out = _u64(0)
        self._check(self._f("fm_index_bytes")(n, sa_sample, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def fm_build(self, BWT, primary: int, SA=None, sa_sample: int = 32, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The index of (BWT, primary) as one np.uint8 blob; SA (the whole suffix array) adds the samples locate needs.  The index
        width follows SA's dtype, else n, unless idx_bits is given.  More than 4 distinct bytes: CapsSaError with code -6."""
        B = self._text(BWT)
        n = int(B.size)
        if idx_bits is None:
            idx_bits = 64 if (SA is not None and np.asarray(SA).dtype.itemsize == 8) or n > 0xFFFFFFFF else 32
        sfx, dt = _sfx(idx_bits)
        if SA is not None:
            SA = np.ascontiguousarray(SA, dtype=dt)
            if SA.size != n:
                raise ValueError("SA must be the whole suffix array: n entries")
        blob = np.zeros(self.fm_index_bytes(n, sa_sample if SA is not None else 0, idx_bits), dtype=np.uint8)
        self._check(self._f(f"fm_build_{sfx}")(B.ctypes.data if n else None, n, int(primary) if n else 0,
                                               SA.ctypes.data if SA is not None else None, sa_sample, blob.ctypes.data, blob.size, device))
        return blob

    def fm_build_device(self, dBWT_ptr: int, n: int, primary: int, dSA_ptr: int, sa_sample: int, dIndex_ptr: int, index_bytes: int,
                        idx_bits: int = 32, stream: int = 0) -> None:
        """The index in device memory: dBWT_ptr (n bytes), dSA_ptr (0: no samples) -> dIndex_ptr (index_bytes >= fm_index_bytes)."""
        sfx, _ = _sfx(idx_bits)
        self._check(self._f(f"fm_build_device_{sfx}")(dBWT_ptr or None, n, int(primary), dSA_ptr or None, sa_sample, dIndex_ptr or None,
                                                      index_bytes, stream or None))

    # ------------------------------------------------------------------ the wide format (include/caps_sa_hip.h "FM-index: the wide format")
    def fm_wide_index_bytes(self, n: int, sigma: int = 0, sa_sample: int = 32, idx_bits: int = 32) -> int:
        """Bytes of the wide index of n symbols over sigma distinct bytes (0: unknown, sized for 256)."""
        out = _u64(0)
        self._check(self._f("fm_wide_index_bytes")(n, sigma, sa_sample, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def fm_wide_workspace_bytes(self, n: int, idx_bits: int = 32) -> int:
        """Device workspace of fm_build_wide_device: two code buffers of n + 1 bytes and the tile counts."""
        out = _u64(0)
        self._check(self._f("fm_wide_workspace_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def fm_build_wide(self, BWT, primary: int, SA=None, sa_sample: int = 32, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The wide index of (BWT, primary), 1 .. 256 distinct bytes, as one np.uint8 blob; arguments as for fm_build."""
        B = self._text(BWT)
        n = int(B.size)
        if idx_bits is None:
            idx_bits = 64 if (SA is not None and np.asarray(SA).dtype.itemsize == 8) or n > 0xFFFFFFFF else 32
        sfx, dt = _sfx(idx_bits)
        if SA is not None:
            SA = np.ascontiguousarray(SA, dtype=dt)
            if SA.size != n:
                raise ValueError("SA must be the whole suffix array: n entries")
        sigma = int(np.unique(B).size) if n else 1
        blob = np.zeros(self.fm_wide_index_bytes(n, sigma, sa_sample if SA is not None else 0, idx_bits), dtype=np.uint8)
        self._check(self._f(f"fm_build_wide_{sfx}")(B.ctypes.data if n else None, n, int(primary) if n else 0,
                                                    SA.ctypes.data if SA is not None else None, sa_sample, blob.ctypes.data, blob.size, device))
        total = int(blob[:256].view(np.uint64)[18])
        assert total == blob.size, (total, blob.size)
        return blob

    def fm_build_wide_device(self, dBWT_ptr: int, n: int, primary: int, dSA_ptr: int, sa_sample: int, dIndex_ptr: int, index_capacity: int,
                             dWS_ptr: int = 0, ws_bytes: int = 0, idx_bits: int = 32, stream: int = 0) -> None:
        """The wide index in device memory; its size is header word 18 (at most fm_wide_index_bytes(n, 0, ..)).  Workspace dWS_ptr of
        ws_bytes (fm_wide_workspace_bytes), or 0: allocated and freed by the call."""
        sfx, _ = _sfx(idx_bits)
        self._check(self._f(f"fm_build_wide_device_{sfx}")(dBWT_ptr or None, n, int(primary), dSA_ptr or None, sa_sample, dIndex_ptr or None,
                                                           index_capacity, dWS_ptr or None, ws_bytes, stream or None))

    def fm_from_bwt_workspace_bytes(self, n: int, sa_sample: int = 32, idx_bits: int = 32) -> int:
        """Device workspace of fm_build_from_bwt_device: one entry per sample and O(n / 64) list nodes, no array of n entries."""
        out = _u64(0)
        self._check(self._f("fm_from_bwt_workspace_bytes")(n, sa_sample, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def fm_build_from_bwt(self, BWT, primary: int, sa_sample: int = 32, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The index WITH samples from (BWT, primary) alone: the same blob as fm_build with the suffix array of the text the BWT
        inverts to.  The index width follows n unless idx_bits is given.  Not the BWT of any text: CapsSaError with code -1; more
        than 4 distinct bytes: -6."""
        B = self._text(BWT)
        n = int(B.size)
        idx_bits = idx_bits or (32 if n <= 0xFFFFFFFF else 64)
        sfx, _ = _sfx(idx_bits)
        blob = np.zeros(self.fm_index_bytes(n, sa_sample, idx_bits), dtype=np.uint8)
        self._check(self._f(f"fm_build_from_bwt_{sfx}")(B.ctypes.data if n else None, n, int(primary) if n else 0, sa_sample,
                                                        blob.ctypes.data, blob.size, device))
        return blob

    def fm_build_from_bwt_device(self, dBWT_ptr: int, n: int, primary: int, sa_sample: int, dIndex_ptr: int, index_bytes: int,
                                 dWS_ptr: int = 0, ws_bytes: int = 0, idx_bits: int = 32, stream: int = 0) -> None:
        """The same in device memory: dBWT_ptr (n bytes) -> dIndex_ptr (index_bytes >= fm_index_bytes(n, sa_sample)); workspace
        dWS_ptr of ws_bytes (fm_from_bwt_workspace_bytes), or 0: allocated and freed by the call."""
        sfx, _ = _sfx(idx_bits)
        self._check(self._f(f"fm_build_from_bwt_device_{sfx}")(dBWT_ptr or None, n, int(primary), sa_sample, dIndex_ptr or None,
                                                               index_bytes, dWS_ptr or None, ws_bytes, stream or None))

    @staticmethod
    def _patterns(patterns):
        """A list of bytes / np.uint8 arrays -> (concatenated bytes, u64 offsets[q + 1])."""
        arrs = [np.frombuffer(bytes(p), dtype=np.uint8) if isinstance(p, (bytes, bytearray)) else np.ascontiguousarray(p, dtype=np.uint8)
                for p in patterns]
        off = np.zeros(len(arrs) + 1, dtype=np.uint64)
        if arrs:
            off[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        cat = np.concatenate(arrs) if arrs and int(off[-1]) else np.zeros(0, dtype=np.uint8)
        return cat, off

    def fm_count(self, index: np.ndarray, patterns, device: int = 0):
        """(first, count) as np.uint64 arrays for a list of patterns (bytes / np.uint8 arrays), or for (bytes, offsets) given as a
        tuple: occurrences of pattern j = SA[first[j] : first[j] + count[j]]."""
        cat, off = patterns if isinstance(patterns, tuple) else self._patterns(patterns)
        cat = np.ascontiguousarray(cat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        q = off.size - 1
        first = np.zeros(q, dtype=np.uint64)
        count = np.zeros(q, dtype=np.uint64)
        self._check(self._f("fm_count")(index.ctypes.data, index.size, cat.ctypes.data if cat.size else None, off.ctypes.data, q,
                                        first.ctypes.data, count.ctypes.data, device))
        return first, count

    def fm_locate(self, index: np.ndarray, first, count, out_off=None, device: int = 0):
        """Positions of the ranks first[j] + t, t < min(count[j], out_off[j + 1] - out_off[j]) -> (pos u64[out_off[q]], out_off);
        out_off = None: every hit of every query."""
        first = np.ascontiguousarray(first, dtype=np.uint64)
        count = np.ascontiguousarray(count, dtype=np.uint64)
        q = first.size
        if out_off is None:
            out_off = np.zeros(q + 1, dtype=np.uint64)
            out_off[1:] = np.cumsum(count, dtype=np.uint64)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64)
        pos = np.full(int(out_off[-1]) if q else 0, 2**64 - 1, dtype=np.uint64)
        self._check(self._f("fm_locate")(index.ctypes.data, index.size, first.ctypes.data, count.ctypes.data, out_off.ctypes.data, q,
                                         pos.ctypes.data if pos.size else None, device))
        return pos, out_off

    def fm_count_device(self, dIndex_ptr: int, index_bytes: int, dPat_ptr: int, dPatOff_ptr: int, q: int, dFirst_ptr: int, dCount_ptr: int,
                        stream: int = 0) -> None:
        self._check(self._f("fm_count_device")(dIndex_ptr or None, index_bytes, dPat_ptr or None, dPatOff_ptr or None, q, dFirst_ptr or None,
                                               dCount_ptr or None, stream or None))

    def fm_locate_device(self, dIndex_ptr: int, index_bytes: int, dFirst_ptr: int, dCount_ptr: int, dOutOff_ptr: int, q: int, dPos_ptr: int,
                         stream: int = 0) -> None:
        self._check(self._f("fm_locate_device")(dIndex_ptr or None, index_bytes, dFirst_ptr or None, dCount_ptr or None, dOutOff_ptr or None, q,
                                                dPos_ptr or None, stream or None))

    # ------------------------------------------------------------------ FM-index: extract (include/caps_sa_hip.h "FM-index: extract")
    def fm_index_bytes_ex(self, n: int, sa_sample: int = 32, text_sample: int = 32, idx_bits: int = 32) -> int:
        """Bytes of the version-2 index of n symbols: SA samples every sa_sample, text-position samples every text_sample."""
        out = _u64(0)
        self._check(self._f("fm_index_bytes_ex")(n, sa_sample, text_sample, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def fm_add_text_samples(self, index: np.ndarray, text_sample: int = 32, device: int = 0) -> np.ndarray:
        """A NEW version-2 blob from a blob with SA samples (version 1, or version 2 at another distance): the blob extract needs."""
        index = np.ascontiguousarray(index, dtype=np.uint8)
        if index.size < 256:
            raise ValueError("not an FM-index blob")
        hdr = index[:256].view(np.uint64)
        n, s, W, v1 = int(hdr[2]), int(hdr[12]), int(hdr[4]), int(hdr[18])
        need = self.fm_index_bytes_ex(n, s, text_sample, 8 * W) if s and W in (4, 8) else index.size
        blob = np.zeros(max(need, index.size), dtype=np.uint8)
        blob[:index.size] = index
        self._check(self._f("fm_add_text_samples")(blob.ctypes.data, blob.size, text_sample, device))
        assert need >= v1
        return blob[:need].copy() if blob.size != need else blob

    def fm_add_text_samples_device(self, dIndex_ptr: int, index_bytes: int, text_sample: int = 32, stream: int = 0) -> None:
        """In place in device memory: index_bytes is the capacity at dIndex_ptr (>= fm_index_bytes_ex)."""
        self._check(self._f("fm_add_text_samples_device")(dIndex_ptr or None, index_bytes, text_sample, stream or None))

    def fm_extract_workspace_bytes(self, q: int) -> int:
        out = _u64(0)
        self._check(self._f("fm_extract_workspace_bytes")(q, ctypes.byref(out)))
        return out.value

    def fm_extract(self, index: np.ndarray, starts, lengths, device: int = 0):
        """(text np.uint8[sum of lengths], out_off u64[q + 1]): text[out_off[j] : out_off[j + 1]] = T[starts[j] : starts[j] + lengths[j]]."""
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
        if starts.shape != lengths.shape or starts.ndim != 1:
            raise ValueError("starts and lengths: two 1-d arrays of one size")
        q = starts.size
        out_off = np.zeros(q + 1, dtype=np.uint64)
        out_off[1:] = np.cumsum(lengths, dtype=np.uint64)
        text = np.zeros(int(out_off[-1]), dtype=np.uint8)
        self._check(self._f("fm_extract")(index.ctypes.data, index.size, starts.ctypes.data if q else None, out_off.ctypes.data, q,
                                          text.ctypes.data if text.size else None, device))
        return text, out_off

    def fm_extract_device(self, dIndex_ptr: int, index_bytes: int, dStart_ptr: int, dOutOff_ptr: int, q: int, dText_ptr: int,
                          dWS_ptr: int = 0, ws_bytes: int = 0, stream: int = 0) -> None:
        """Device arrays: dStart u64[q], dOutOff u64[q + 1], dText u8[dOutOff[q]]; workspace dWS_ptr of ws_bytes
        (fm_extract_workspace_bytes), or 0: allocated and freed by the call."""
        self._check(self._f("fm_extract_device")(dIndex_ptr or None, index_bytes, dStart_ptr or None, dOutOff_ptr or None, q,
                                                 dText_ptr or None, dWS_ptr or None, ws_bytes, stream or None))

    # ------------------------------------------------------------------ FM-index: matching statistics and MEMs
    def fm_match(self, index: np.ndarray, patterns, max_len: int = 0, intervals: bool = False, device: int = 0):
        """(len np.uint32[total], first, count, pat_off): slot pat_off[j] - pat_off[0] + e - 1 holds L[e] of pattern j, the longest
        piece ending at e that occurs in the text (at most max_len when max_len > 0); first / count (np.uint64, its SA interval) are
        None unless intervals.  patterns as for fm_count."""
        cat, off = patterns if isinstance(patterns, tuple) else self._patterns(patterns)
        cat = np.ascontiguousarray(cat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        q = off.size - 1
        total = int(off[-1] - off[0]) if q > 0 else 0
        ln = np.zeros(total, dtype=np.uint32)
        first = np.zeros(total, dtype=np.uint64) if intervals else None
        count = np.zeros(total, dtype=np.uint64) if intervals else None
        self._check(self._f("fm_match")(index.ctypes.data, index.size, cat.ctypes.data if cat.size else None, off.ctypes.data, q, max_len,
                                        ln.ctypes.data, first.ctypes.data if intervals else None, count.ctypes.data if intervals else None,
                                        device))
        return ln, first, count, off

    def fm_match_device(self, dIndex_ptr: int, index_bytes: int, dPat_ptr: int, dPatOff_ptr: int, q: int, max_len: int, dLen_ptr: int,
                        dFirst_ptr: int = 0, dCount_ptr: int = 0, stream: int = 0) -> None:
        """Device arrays: dPatOff u64[q + 1], dLen u32[total], dFirst / dCount u64[total] or 0 (not written)."""
        self._check(self._f("fm_match_device")(dIndex_ptr or None, index_bytes, dPat_ptr or None, dPatOff_ptr or None, q, max_len,
                                               dLen_ptr or None, dFirst_ptr or None, dCount_ptr or None, stream or None))

    def fm_mems_workspace_bytes(self, total_pattern_bytes: int, q: int) -> int:
        out = _u64(0)
        self._check(self._f("fm_mems_workspace_bytes")(total_pattern_bytes, q, ctypes.byref(out)))
        return out.value

    def fm_mems(self, index: np.ndarray, patterns, min_len: int = 1, device: int = 0):
        """(records, mem_off): the maximal exact matches of at least min_len bytes as a structured array (MEM_DTYPE: pattern, start,
        length, first, count) in (pattern, increasing end) order; records[mem_off[j] : mem_off[j + 1]] are pattern j's.  The
        counting call, then the writing call."""
        cat, off = patterns if isinstance(patterns, tuple) else self._patterns(patterns)
        cat = np.ascontiguousarray(cat, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        q = off.size - 1
        mem_off = np.zeros(q + 1, dtype=np.uint64)
        args = (index.ctypes.data, index.size, cat.ctypes.data if cat.size else None, off.ctypes.data, q, min_len, mem_off.ctypes.data)
        self._check(self._f("fm_mems")(*args, None, 0, device))
        mems = np.zeros(int(mem_off[-1]), dtype=MEM_DTYPE)
        if mems.size:
            self._check(self._f("fm_mems")(*args, mems.ctypes.data, mems.size, device))
        return mems, mem_off

    def fm_mems_device(self, dIndex_ptr: int, index_bytes: int, dPat_ptr: int, dPatOff_ptr: int, q: int, min_len: int, dMemOff_ptr: int,
                       dMems_ptr: int = 0, mem_capacity: int = 0, dWS_ptr: int = 0, ws_bytes: int = 0, stream: int = 0) -> None:
        """Device arrays: dMemOff u64[q + 1] (always written), dMems 32-byte records or 0 (the counting call); workspace dWS_ptr of
        ws_bytes (fm_mems_workspace_bytes), or 0: allocated and freed by the call."""
        self._check(self._f("fm_mems_device")(dIndex_ptr or None, index_bytes, dPat_ptr or None, dPatOff_ptr or None, q, min_len,
                                              dMemOff_ptr or None, dMems_ptr or None, mem_capacity, dWS_ptr or None, ws_bytes, stream or None))

    # ------------------------------------------------------------------ k-mers (include/caps_sa_hip.h "k-mers from SA and LCP")
    @staticmethod
    def _sa_lcp(SA, LCP, idx_bits):
        """(SA, LCP, n, suffix): both contiguous in one index dtype -- SA's own unless idx_bits is given."""
        SA = np.asarray(SA)
        if idx_bits is None:
            idx_bits = 64 if SA.dtype.itemsize == 8 else 32
        sfx, dt = _sfx(idx_bits)
        SA = np.ascontiguousarray(SA, dtype=dt)
        LCP = np.ascontiguousarray(LCP, dtype=dt)
        if SA.ndim != 1 or SA.shape != LCP.shape:
            raise ValueError("SA and LCP: two 1-d arrays of one size")
        return SA, LCP, int(SA.size), sfx

    def kmer_workspace_bytes(self, n: int, idx_bits: int = 32) -> int:
        out = _u64(0)
        self._check(self._f("kmer_workspace_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def kmers(self, SA, LCP, k: int, min_count: int = 1, max_count: int = 0, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The distinct k-mers with min_count <= count (<= max_count unless that is 0) as a structured array (KMER_DTYPE: first,
        count, pos) in the library's byte order: k-mer j is T[pos : pos + k] and occurs at SA[first : first + count].  The counting
        call, then the writing call."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        found = _u64(0)
        args = (SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n, k, min_count, max_count)
        self._check(self._f(f"kmers_{sfx}")(*args, None, 0, ctypes.byref(found), device))
        rec = np.zeros(found.value, dtype=KMER_DTYPE)
        if rec.size:
            self._check(self._f(f"kmers_{sfx}")(*args, rec.ctypes.data, rec.size, ctypes.byref(found), device))
        return rec

    def kmer_spectrum(self, SA, LCP, k: int, bins: int = 1024, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """np.uint64[bins + 1]: hist[c] = the distinct k-mers that occur c times, hist[bins] = bins times or more, hist[0] = 0."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        hist = np.zeros(max(int(bins), 0) + 1, dtype=np.uint64)
        self._check(self._f(f"kmer_spectrum_{sfx}")(SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n, k, bins,
                                                    hist.ctypes.data, device))
        return hist

    def kmer_census(self, SA, LCP, max_k: int, idx_bits: int | None = None, device: int = 0):
        """(distinct, unique), np.uint64[max_k + 1] each: the number of distinct k-mers and of those that occur once, k = 1 .. max_k."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        distinct = np.zeros(max(int(max_k), 0) + 1, dtype=np.uint64)
        unique = np.zeros_like(distinct)
        self._check(self._f(f"kmer_census_{sfx}")(SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n, max_k,
                                                  distinct.ctypes.data, unique.ctypes.data, device))
        return distinct, unique

    def kmers_device(self, dSA_ptr: int, dLCP_ptr: int, n: int, k: int, min_count: int = 1, max_count: int = 0, dRecords_ptr: int = 0,
                     capacity: int = 0, dWS_ptr: int = 0, ws_bytes: int = 0, idx_bits: int = 32, stream: int = 0) -> int:
        """Device arrays -> the number of records; dRecords_ptr 0: the counting call, else `capacity` 24-byte records are written
        there.  More records than capacity: CapsSaError (code -1) whose n_records attribute holds their number."""
        sfx, _ = _sfx(idx_bits)
        found = _u64(0)
        rc = self._f(f"kmers_device_{sfx}")(dSA_ptr or None, dLCP_ptr or None, n, k, min_count, max_count, dRecords_ptr or None, capacity,
                                            ctypes.byref(found), dWS_ptr or None, ws_bytes, stream or None)
        if rc != 0:
            err = CapsSaError(rc, self._f("last_error")().decode(errors="replace"))
            err.n_records = found.value
            raise err
        return found.value

    def kmer_spectrum_device(self, dSA_ptr: int, dLCP_ptr: int, n: int, k: int, bins: int = 1024, dWS_ptr: int = 0, ws_bytes: int = 0,
                             idx_bits: int = 32, stream: int = 0) -> np.ndarray:
        sfx, _ = _sfx(idx_bits)
        hist = np.zeros(max(int(bins), 0) + 1, dtype=np.uint64)
        self._check(self._f(f"kmer_spectrum_device_{sfx}")(dSA_ptr or None, dLCP_ptr or None, n, k, bins, hist.ctypes.data, dWS_ptr or None,
                                                           ws_bytes, stream or None))
        return hist

    def kmer_census_device(self, dSA_ptr: int, dLCP_ptr: int, n: int, max_k: int, dWS_ptr: int = 0, ws_bytes: int = 0, idx_bits: int = 32,
                           stream: int = 0):
        sfx, _ = _sfx(idx_bits)
        distinct = np.zeros(max(int(max_k), 0) + 1, dtype=np.uint64)
        unique = np.zeros_like(distinct)
        self._check(self._f(f"kmer_census_device_{sfx}")(dSA_ptr or None, dLCP_ptr or None, n, max_k, distinct.ctypes.data,
                                                         unique.ctypes.data, dWS_ptr or None, ws_bytes, stream or None))
        return distinct, unique

    # ------------------------------------------------------------------ MUMs and MEMs between two texts (include/caps_sa_hip.h)
    def cross_workspace_bytes(self, n: int, idx_bits: int = 32) -> int:
        out = _u64(0)
        self._check(self._f("cross_workspace_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    @staticmethod
    def cross_summary(words) -> dict:
        """The 8 summary words of a cross call as a dict."""
        w = [int(x) for x in words]
        return {"records": w[0], "skipped_runs": w[1], "lcs_len": w[2], "lcs_a": w[3], "lcs_b": w[4]}

    def _cross(self, which: str, SA, LCP, BWT, split: int, min_len: int, max_occ, idx_bits, device: int):
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        BWT = np.ascontiguousarray(np.frombuffer(BWT, dtype=np.uint8) if isinstance(BWT, (bytes, bytearray)) else BWT, dtype=np.uint8)
        if BWT.shape != SA.shape:
            raise ValueError("BWT: one byte per rank")
        summary = np.zeros(8, dtype=np.uint64)
        args = (SA.ctypes.data if n else None, LCP.ctypes.data if n else None, BWT.ctypes.data if n else None, n, split, min_len)
        if which == "mems":
            args += (max_occ,)
        f = self._f(f"cross_{which}_{sfx}")
        self._check(f(*args, None, 0, summary.ctypes.data, device))
        rec = np.zeros(int(summary[0]), dtype=CROSS_DTYPE)
        if rec.size:
            self._check(f(*args, rec.ctypes.data, rec.size, summary.ctypes.data, device))
        return rec, summary

    def cross_mums(self, SA, LCP, BWT, split: int, min_len: int = 1, idx_bits: int | None = None, device: int = 0):
        """(records, summary): the maximal unique matches between T[:split] and T[split:] as a structured array (CROSS_DTYPE: a, b,
        len) in rank order, and the 8 summary words.  The counting call, then the writing call."""
        return self._cross("mums", SA, LCP, BWT, split, min_len, None, idx_bits, device)

    def cross_mems(self, SA, LCP, BWT, split: int, min_len: int = 1, max_occ: int = CROSS_MAX_OCC, idx_bits: int | None = None,
                   device: int = 0):
        """(records, summary): the maximal exact matches whose first min_len bytes occur at most max_occ times in T, ordered by the
        upper rank q ascending, then the lower rank p descending; summary[1] counts the runs skipped as too frequent."""
        return self._cross("mems", SA, LCP, BWT, split, min_len, max_occ, idx_bits, device)

    def cross_device(self, which: str, dSA_ptr: int, dLCP_ptr: int, dBWT_ptr: int, n: int, split: int, min_len: int, max_occ: int = CROSS_MAX_OCC,
                     dRecords_ptr: int = 0, capacity: int = 0, dWS_ptr: int = 0, ws_bytes: int = 0, idx_bits: int = 32, stream: int = 0) -> np.ndarray:
        """Device arrays -> the 8 summary words; which: "mums" or "mems".  dRecords_ptr 0: the counting call, else `capacity`
        24-byte records may be written there.  More records than capacity: CapsSaError (code -1) whose summary attribute holds the
        words."""
        sfx, _ = _sfx(idx_bits)
        summary = np.zeros(8, dtype=np.uint64)
        args = (dSA_ptr or None, dLCP_ptr or None, dBWT_ptr or None, n, split, min_len)
        if which == "mems":
            args += (max_occ,)
        rc = self._f(f"cross_{which}_device_{sfx}")(*args, dRecords_ptr or None, capacity, summary.ctypes.data, dWS_ptr or None, ws_bytes,
                                                    stream or None)
        if rc != 0:
            err = CapsSaError(rc, self._f("last_error")().decode(errors="replace"))
            err.summary = summary
            raise err
        return summary

    # ------------------------------------------------------------------ k-mers across a collection (include/caps_sa_hip.h)
    def coll_workspace_bytes(self, n: int, idx_bits: int = 32) -> int:
        out = _u64(0)
        self._check(self._f("coll_workspace_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    @staticmethod
    def coll_docs(docs):
        """A sequence of (start, length) -> (starts, lengths, m): two np.uint64 arrays for the doc_start / doc_len arguments."""
        d = np.asarray(list(docs), dtype=np.uint64).reshape(-1, 2)
        return np.ascontiguousarray(d[:, 0]), np.ascontiguousarray(d[:, 1]), int(d.shape[0])

    def coll_kmers(self, SA, LCP, k: int, docs, min_docs: int = 1, max_docs: int = 0, all_of: int = 0, none_of: int = 0,
                   idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The collection k-mers that pass the filter as a structured array (COLL_DTYPE: first, count, occ, docs) in the library's byte
        order; docs: a sequence of (start, length).  The counting call, then the writing call."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        st, ln, m = self.coll_docs(docs)
        found = _u64(0)
        args = (SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n, k, st.ctypes.data, ln.ctypes.data, m, min_docs, max_docs,
                all_of, none_of)
        self._check(self._f(f"coll_kmers_{sfx}")(*args, None, 0, ctypes.byref(found), device))
        rec = np.zeros(found.value, dtype=COLL_DTYPE)
        if rec.size:
            self._check(self._f(f"coll_kmers_{sfx}")(*args, rec.ctypes.data, rec.size, ctypes.byref(found), device))
        return rec

    def coll_sharing(self, SA, LCP, k: int, docs, idx_bits: int | None = None, device: int = 0):
        """(freq, shared): np.uint64[65] and np.uint64[m, m] -- freq[c] = the collection k-mers in exactly c documents, shared[a, b] =
        those in both a and b."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        st, ln, m = self.coll_docs(docs)
        freq = np.zeros(COLL_MAX_DOCS + 1, dtype=np.uint64)
        shared = np.zeros((max(m, 1), max(m, 1)), dtype=np.uint64)
        self._check(self._f(f"coll_sharing_{sfx}")(SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n, k, st.ctypes.data,
                                                   ln.ctypes.data, m, freq.ctypes.data, shared.ctypes.data, device))
        return freq, shared

    def coll_kmers_device(self, dSA_ptr: int, dLCP_ptr: int, n: int, k: int, docs, min_docs: int = 1, max_docs: int = 0, all_of: int = 0,
                          none_of: int = 0, dRecords_ptr: int = 0, capacity: int = 0, dWS_ptr: int = 0, ws_bytes: int = 0, idx_bits: int = 32,
                          stream: int = 0) -> int:
        """Device arrays -> the number of records; dRecords_ptr 0: the counting call, else `capacity` 32-byte records may be written
        there.  More records than capacity: CapsSaError (code -1) whose n_records attribute holds their number."""
        sfx, _ = _sfx(idx_bits)
        st, ln, m = self.coll_docs(docs)
        found = _u64(0)
        rc = self._f(f"coll_kmers_device_{sfx}")(dSA_ptr or None, dLCP_ptr or None, n, k, st.ctypes.data, ln.ctypes.data, m, min_docs, max_docs,
                                                 all_of, none_of, dRecords_ptr or None, capacity, ctypes.byref(found), dWS_ptr or None, ws_bytes,
                                                 stream or None)
        if rc != 0:
            err = CapsSaError(rc, self._f("last_error")().decode(errors="replace"))
            err.n_records = found.value
            raise err
        return found.value

    def coll_sharing_device(self, dSA_ptr: int, dLCP_ptr: int, n: int, k: int, docs, dWS_ptr: int = 0, ws_bytes: int = 0, idx_bits: int = 32,
                            stream: int = 0):
        sfx, _ = _sfx(idx_bits)
        st, ln, m = self.coll_docs(docs)
        freq = np.zeros(COLL_MAX_DOCS + 1, dtype=np.uint64)
        shared = np.zeros((max(m, 1), max(m, 1)), dtype=np.uint64)
        self._check(self._f(f"coll_sharing_device_{sfx}")(dSA_ptr or None, dLCP_ptr or None, n, k, st.ctypes.data, ln.ctypes.data, m,
                                                          freq.ctypes.data, shared.ctypes.data, dWS_ptr or None, ws_bytes, stream or None))
        return freq, shared

    # ------------------------------------------------------------------ LPF and LZ77 (include/caps_sa_hip.h "LPF and LZ77 from SA and LCP")
    def lpf_workspace_bytes(self, n: int, idx_bits: int = 32) -> int:
        out = _u64(0)
        self._check(self._f("lpf_workspace_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def lz77_workspace_bytes(self, n: int, idx_bits: int = 32) -> int:
        out = _u64(0)
        self._check(self._f("lz77_workspace_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def lpf(self, SA, LCP, idx_bits: int | None = None, device: int = 0):
        """(LPF, Prev) in text order, in the index dtype: LPF[i] = the longest prefix of T[i:] that also starts at some j < i, Prev[i]
        = such a j (all ones where LPF[i] = 0)."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        LPF = np.zeros(n, dtype=SA.dtype)
        Prev = np.full(n, np.iinfo(SA.dtype).max, dtype=SA.dtype)
        self._check(self._f(f"lpf_{sfx}")(SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n, LPF.ctypes.data if n else None,
                                          Prev.ctypes.data if n else None, device))
        return LPF, Prev

    def lz77(self, SA, LCP, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The LZ77 factorization as a structured array (LZ_DTYPE: pos, len, src) in text order; src = LZ_LITERAL: a literal of one
        byte.  One host call (arrays up, lpf, count, write) into a buffer of min(n, n / 8 + 1024) records, which holds the parse of any
        text whose phrases average 8 bytes or more; only where it does not, a second call with the exact number, which uploads the arrays
        and runs lpf again (a caller with the arrays on the device uses lpf_device and lz77_device and pays for lpf once)."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        found = _u64(0)
        args = (SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n)
        f = self._f(f"lz77_{sfx}")
        rec = np.zeros(min(n, n // 8 + 1024), dtype=LZ_DTYPE)
        rc = f(*args, rec.ctypes.data if rec.size else None, rec.size, ctypes.byref(found), device)
        if rc != 0 and found.value > rec.size:               # the buffer was too small: the number is valid, nothing was written
            rec = np.zeros(found.value, dtype=LZ_DTYPE)
            rc = f(*args, rec.ctypes.data, rec.size, ctypes.byref(found), device)
        self._check(rc)
        return rec[:found.value].copy() if found.value < rec.size else rec

    def lpf_device(self, dSA_ptr: int, dLCP_ptr: int, n: int, dLPF_ptr: int = 0, dPrev_ptr: int = 0, dWS_ptr: int = 0, ws_bytes: int = 0,
                   idx_bits: int = 32, stream: int = 0) -> None:
        """Device arrays -> LPF and Prev (n entries of the index width each, text order; 0: not written)."""
        sfx, _ = _sfx(idx_bits)
        self._check(self._f(f"lpf_device_{sfx}")(dSA_ptr or None, dLCP_ptr or None, n, dLPF_ptr or None, dPrev_ptr or None, dWS_ptr or None,
                                                 ws_bytes, stream or None))

    def lz77_device(self, dLPF_ptr: int, dPrev_ptr: int, n: int, dRecords_ptr: int = 0, capacity: int = 0, dWS_ptr: int = 0,
                    ws_bytes: int = 0, idx_bits: int = 32, stream: int = 0) -> int:
        """Device LPF and Prev -> the number of phrases; dRecords_ptr 0: the counting call, else `capacity` 24-byte records are written
        there.  More phrases than capacity: CapsSaError (code -1) whose n_phrases attribute holds their number."""
        sfx, _ = _sfx(idx_bits)
        found = _u64(0)
        rc = self._f(f"lz77_device_{sfx}")(dLPF_ptr or None, dPrev_ptr or None, n, dRecords_ptr or None, capacity, ctypes.byref(found),
                                           dWS_ptr or None, ws_bytes, stream or None)
        if rc != 0:
            err = CapsSaError(rc, self._f("last_error")().decode(errors="replace"))
            err.n_phrases = found.value
            raise err
        return found.value

    # ------------------------------------------------------------------ ISA and the LCE index (include/caps_sa_hip.h "ISA and longest common extensions")
    def isa(self, SA, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The inverse suffix array, ISA[SA[r]] = r, in SA's dtype (or idx_bits).  Not a permutation of 0 .. n - 1: CapsSaError (-1)."""
        SA = np.asarray(SA)
        sfx, dt = _sfx(idx_bits or (64 if SA.dtype.itemsize == 8 else 32))
        SA = np.ascontiguousarray(SA, dtype=dt)
        if SA.ndim != 1:
            raise ValueError("SA: a 1-d array")
        n = int(SA.size)
        ISA = np.zeros(n, dtype=dt)
        self._check(self._f(f"isa_{sfx}")(SA.ctypes.data if n else None, n, ISA.ctypes.data if n else None, device))
        return ISA

    def isa_device(self, dSA_ptr: int, n: int, dISA_ptr: int, idx_bits: int = 32, stream: int = 0) -> None:
        sfx, _ = _sfx(idx_bits)
        self._check(self._f(f"isa_device_{sfx}")(dSA_ptr or None, n, dISA_ptr or None, stream or None))

    def lce_index_bytes(self, n: int, idx_bits: int = 32) -> int:
        out = _u64(0)
        self._check(self._f("lce_index_bytes")(n, idx_bits // 8, ctypes.byref(out)))
        return out.value

    def lce_build(self, SA, LCP, idx_bits: int | None = None, device: int = 0) -> np.ndarray:
        """The LCE index of (SA, LCP) as one np.uint8 blob: ISA, LCP and the two tiers of range-minimum tables."""
        SA, LCP, n, sfx = self._sa_lcp(SA, LCP, idx_bits)
        blob = np.zeros(self.lce_index_bytes(n, SA.dtype.itemsize * 8), dtype=np.uint8)
        self._check(self._f(f"lce_build_{sfx}")(SA.ctypes.data if n else None, LCP.ctypes.data if n else None, n, blob.ctypes.data, blob.size, device))
        return blob

    def lce_build_device(self, dSA_ptr: int, dLCP_ptr: int, n: int, dIndex_ptr: int, index_bytes: int, idx_bits: int = 32, stream: int = 0) -> None:
        sfx, _ = _sfx(idx_bits)
        self._check(self._f(f"lce_build_device_{sfx}")(dSA_ptr or None, dLCP_ptr or None, n, dIndex_ptr or None, index_bytes, stream or None))

    def _lce_pairs(self, name, index, a, b, extra, device):
        index = np.ascontiguousarray(index, dtype=np.uint8)
        a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
        b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1)
        if a.size != b.size:
            raise ValueError("two arrays of one size")
        q = int(a.size)
        out = np.zeros(q, dtype=np.uint64)
        self._check(self._f(name)(index.ctypes.data, index.size, a.ctypes.data if q else None, b.ctypes.data if q else None, q, *extra,
                                  out.ctypes.data if q else None, device))
        return out

    def lce_range_min(self, index: np.ndarray, lo, hi, device: int = 0) -> np.ndarray:
        """min LCP[lo[x] .. hi[x]] over RANKS, both ends inclusive, as np.uint64; lo > hi or hi >= n: CapsSaError (-1)."""
        return self._lce_pairs("lce_range_min", index, lo, hi, (), device)

    def lce(self, index: np.ndarray, i, j, mismatches: int = 0, device: int = 0) -> np.ndarray:
        """The longest common extension of T[i[x]:] and T[j[x]:] with at most `mismatches` (0 .. 1024) differing places, np.uint64."""
        if mismatches < 0:
            raise ValueError("mismatches: 0 .. 1024")
        return self._lce_pairs("lce", index, i, j, (int(mismatches),), device)

    def lce_range_min_device(self, dIndex_ptr: int, index_bytes: int, dLo_ptr: int, dHi_ptr: int, q: int, dMin_ptr: int, stream: int = 0) -> None:
        self._check(self._f("lce_range_min_device")(dIndex_ptr or None, index_bytes, dLo_ptr or None, dHi_ptr or None, q, dMin_ptr or None,
                                                    stream or None))

    def lce_device(self, dIndex_ptr: int, index_bytes: int, dI_ptr: int, dJ_ptr: int, q: int, mismatches: int, dLen_ptr: int, stream: int = 0) -> None:
        self._check(self._f("lce_device")(dIndex_ptr or None, index_bytes, dI_ptr or None, dJ_ptr or None, q, mismatches, dLen_ptr or None,
                                          stream or None))

    # ------------------------------------------------------------------ kernel-level entry points
    def sort_suffixes(self, T, idx, idx_bits: int = 32, device: int = 0):
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        idx = np.ascontiguousarray(idx, dtype=dt)
        out_sa = np.empty_like(idx)
        out_lcp = np.empty_like(idx)
        self._check(self._f(f"sort_suffixes_{sfx}")(T.ctypes.data, T.size, idx.ctypes.data, idx.size,
                                                    out_sa.ctypes.data, out_lcp.ctypes.data, device))
        return out_sa, out_lcp

    def sort_segments(self, T, idx, seg_start, idx_bits: int = 32, device: int = 0):
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        idx = np.ascontiguousarray(idx, dtype=dt)
        seg = np.ascontiguousarray(seg_start, dtype=np.uint64)
        out_sa = np.empty_like(idx)
        out_lcp = np.empty_like(idx)
        self._check(self._f(f"sort_segments_{sfx}")(T.ctypes.data, T.size, idx.ctypes.data, idx.size, seg.ctypes.data,
                                                    seg.size - 1, out_sa.ctypes.data, out_lcp.ctypes.data, device))
        return out_sa, out_lcp

    def merge(self, T, X, Y, LX, LY, idx_bits: int = 32, device: int = 0):
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        X, Y, LX, LY = (np.ascontiguousarray(v, dtype=dt) for v in (X, Y, LX, LY))
        Z = np.empty(X.size + Y.size, dtype=dt)
        LZ = np.empty_like(Z)
        self._check(self._f(f"merge_{sfx}")(T.ctypes.data, T.size, X.ctypes.data, X.size, Y.ctypes.data, Y.size,
                                            LX.ctypes.data, LY.ctypes.data, Z.ctypes.data, LZ.ctypes.data, device))
        return Z, LZ

    def upper_bound(self, T, X, pivots, idx_bits: int = 32, device: int = 0):
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        X = np.ascontiguousarray(X, dtype=dt)
        pivots = np.ascontiguousarray(pivots, dtype=dt)
        out = np.empty_like(pivots)
        self._check(self._f(f"upper_bound_{sfx}")(T.ctypes.data, T.size, X.ctypes.data, X.size, pivots.ctypes.data,
                                                  pivots.size, out.ctypes.data, device))
        return out

    def lcp(self, T, a, b, idx_bits: int = 32, device: int = 0):
        T = self._text(T)
        sfx, dt = _sfx(idx_bits)
        a = np.ascontiguousarray(a, dtype=dt)
        b = np.ascontiguousarray(b, dtype=dt)
        out = np.empty_like(a)
        self._check(self._f(f"lcp_{sfx}")(T.ctypes.data, T.size, a.ctypes.data, b.ctypes.data, a.size,
                                          out.ctypes.data, device))
        return out


class Shard:
    """One rank of the multi-GPU construction (caps_sa_hip_shard_*, include/caps_sa_hip.h).
    Pointers are raw device addresses (torch tensors' data_ptr())."""

    def __init__(self, lib: CapsLib, dT_ptr: int, n: int, p: int, idx_bits: int, rank: int, world: int, stream: int = 0):
        self.lib = lib
        self.h = _vp(None)
        lib._check(lib._f("shard_create")(dT_ptr, n, p, idx_bits // 8, rank, world, stream or None, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.lib._f("shard_destroy")(self.h)
            self.h = _vp(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        inf = ShardInfo()
        self.lib._check(self.lib._f("shard_info")(self.h, ctypes.byref(inf)))
        return inf.as_dict()

    def phase1(self, d_sample_keys: int, d_sample_sa: int):
        self.lib._check(self.lib._f("shard_phase1")(self.h, d_sample_keys or None, d_sample_sa or None))

    def pivots(self, d_all_keys: int, d_all_sa: int, d_local_sizes: int):
        self.lib._check(self.lib._f("shard_pivots")(self.h, d_all_keys, d_all_sa, d_local_sizes))

    def collate(self, all_sizes: np.ndarray, d_send_keys: int, d_send_sa: int):
        all_sizes = np.ascontiguousarray(all_sizes, dtype=np.uint64)
        world = all_sizes.shape[0]
        sc = np.zeros(world, dtype=np.uint64)
        rc = np.zeros(world, dtype=np.uint64)
        self.lib._check(self.lib._f("shard_collate")(self.h, all_sizes.ctypes.data, d_send_keys or None, d_send_sa or None,
                                                     sc.ctypes.data, rc.ctypes.data))
        return sc, rc

    def phase2(self, d_recv_keys: int, d_recv_sa: int, dSA: int, dLCP: int):
        self.lib._check(self.lib._f("shard_phase2")(self.h, d_recv_keys or None, d_recv_sa or None, dSA or None, dLCP or None))

    def scatter(self, d_send_keys: int, d_send_sa: int, d_report: int):
        self.lib._check(self.lib._f("shard_scatter")(self.h, d_send_keys, d_send_sa, d_report))

    def plan(self, all_reports: np.ndarray):
        """-> (fallback code, send_counts, recv_counts); code 0: go on with the direct path."""
        all_reports = np.ascontiguousarray(all_reports, dtype=np.uint64)
        world = all_reports.shape[0]
        sc = np.zeros(world, dtype=np.uint64)
        rc = np.zeros(world, dtype=np.uint64)
        code = self.lib._f("shard_plan")(self.h, all_reports.ctypes.data, sc.ctypes.data, rc.ctypes.data)
        if code < 0:
            self.lib._check(code)
        return code, sc, rc

    def sort_owned(self, d_recv_keys: int, d_recv_sa: int, dSA: int, dLCP: int) -> int:
        """-> 0, or CAPS_SA_FB_KEY32 (6): a slot overflowed under 32-bit keys; all ranks set_key_bits(64) and start over."""
        code = self.lib._f("shard_sort")(self.h, d_recv_keys or None, d_recv_sa or None, dSA or None, dLCP or None)
        if code < 0:
            self.lib._check(code)
        return code

    def set_key_bits(self, bits: int):
        self.lib._check(self.lib._f("shard_set_key_bits")(self.h, bits))

    def phase1_arrays(self, d_keys_out: int = 0, d_sa_out: int = 0):
        """Copies the rank's sorted subarrays (after phase1()) into the given device buffers; -> (count, subarray length)."""
        c, sl = _u64(0), _u64(0)
        self.lib._check(self.lib._f("shard_phase1_arrays")(self.h, d_keys_out or None, d_sa_out or None, ctypes.byref(c), ctypes.byref(sl)))
        return c.value, sl.value

    def last_sa(self) -> int:
        v = _u64(0)
        self.lib._check(self.lib._f("shard_last_sa")(self.h, ctypes.byref(v)))
        return v.value

    def fix_first_lcp(self, prev_sa: int, dLCP: int):
        self.lib._check(self.lib._f("shard_fix_first_lcp")(self.h, prev_sa, dLCP or None))

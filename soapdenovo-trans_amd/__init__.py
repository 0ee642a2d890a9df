"""soapdenovo-trans_amd -- MI355X-native `pregraph` hashing path of SOAPdenovo-Trans.

The product is ``csrc/libsdt_gpu.so`` (hand-written HIP for gfx950 behind the C ABI declared in
``include/sdt_gpu.h``) plus the C host ``csrc/host`` that keeps the reference's
``pregraph -s cfg -K k -o out`` command line.  This Python package is the thin host-side mirror used by
tests and bench.py: it loads the shared library with ctypes and exposes one class whose methods have
the names and argument meaning of the C ABI.  There is no CPU fallback here: if the library is missing
or no gfx950 device is present the calls raise.

The directory name contains a hyphen, so import it through ``__graft_entry__.load_package()``.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.join(PKG_DIR, "csrc")
LIB_PATH = os.path.join(CSRC_DIR, "libsdt_gpu.so")
REPO_ROOT = os.path.dirname(PKG_DIR)

SDT_FLAG_DIRECT, SDT_FLAG_PARTITION, SDT_FLAG_TRACK_FIRST, SDT_FLAG_KEEP_READS, SDT_FLAG_CONTIG_INDEX = 1, 2, 4, 8, 16
SDT_OK, SDT_EINVAL, SDT_ENODEV, SDT_ENOMEM, SDT_EHIP, SDT_EFULL, SDT_ESTATE, SDT_ELIMIT = 0, -1, -2, -3, -4, -5, -6, -7

# every symbol include/sdt_gpu.h declares: (name, restype, argtypes)
_c = ctypes
_ABI = [
    ("sdt_gpu_init", _c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int, _c.c_uint64, _c.c_uint32]),
    ("sdt_gpu_destroy", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_last_error", _c.c_char_p, []),
    ("sdt_gpu_abi_version", _c.c_int, []),
    ("sdt_gpu_reset", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_push_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_push_reads_async", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_push_reads_fixed_async", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_push_wait", _c.c_int, [_c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_hint_total_kmers", _c.c_int, [_c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_host_alloc", _c.c_void_p, [_c.c_size_t]),
    ("sdt_gpu_host_free", None, [_c.c_void_p]),
    ("sdt_gpu_count_reads_device", _c.c_int,
     [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_uint64]),
    ("sdt_gpu_finish_count", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_shard_cut_ranges", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p]),
    ("sdt_shard_plan", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_uint32, _c.c_uint32] + [_c.c_void_p] * 6),
    ("sdt_kmer_final_bucket", _c.c_int, [_c.c_void_p, _c.c_int]),
    ("sdt_gpu_table_info", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("sdt_sk_plan_count_items", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_uint64, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_uint32,
                                           _c.c_void_p, _c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_delow", _c.c_int, [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_mark_and_hist", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_export_nodes", _c.c_int,
     [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64,
      _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_set_read_ordinal", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64]),
    ("sdt_gpu_load_paths", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                      _c.c_uint64, _c.c_uint64]),
    ("sdt_gpu_export_paths", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_import_paths", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint64]),
    ("sdt_gpu_release_table", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_map_reads", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_export_arcs", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                       _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_set_node_index", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_update_nodes", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_tip_walks", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_tip_walks_compact", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_minor_out_dry", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64),
                                         _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_edge_ports", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_build_host_index", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_build_host_index64", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_set_graph_index_bits", _c.c_int, [_c.c_void_p, _c.c_int]),
    ("sdt_gpu_graph_index_bits", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_layout_sorted_keys", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_layout_apply", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_layout_on_device", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_export_ordered", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_update_nodes_by_index", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_tip_walks_labelled", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_minor_out_labelled", _c.c_int, [_c.c_void_p, _c.c_double, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_fetch_records", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_minor_out_commit", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_fetch_skipped", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_minor_out_commit_begin", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_minor_out_commit_finish", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_fetch_written", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_build_edges", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_fetch_edge_bases", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_index_contigs", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_set_contig_table", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_align_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_int,
                                       _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_align_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p,
                                              _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_key_words", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_table_slots", _c.c_uint64, [_c.c_void_p]),
    ("sdt_gpu_stream", _c.c_void_p, [_c.c_void_p]),
    ("sdt_gpu_set_stream", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_kernel_time", _c.c_int,
     [_c.c_void_p, _c.c_int, _c.POINTER(_c.c_double), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_stage_times", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_double), _c.POINTER(_c.c_uint64)]),
    ("sdt_owner_hash", _c.c_uint64, [_c.c_void_p, _c.c_int]),
    ("sdt_gpu_comm_id", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_comm_init", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int]),
    ("sdt_gpu_comm_init_shm", _c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_int, _c.c_int]),
    ("sdt_gpu_count_reads_sharded", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_uint64]),
    ("sdt_gpu_push_reads_sharded", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_allreduce_i64", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
    ("sdt_gpu_comm_stats", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_double),
                                      _c.POINTER(_c.c_uint64)]),
    ("sdt_kmer_owner", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int]),
    ("sdt_kmer_bucket", _c.c_int, [_c.c_void_p, _c.c_int]),
    ("sdt_gpu_shard_ranges", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("sdt_comm_selftest_shm", _c.c_int, [_c.c_char_p, _c.c_int, _c.c_int, _c.c_int]),
    ("sdt_gpu_import_nodes", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_keep_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_search_kmers", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_search_kmers_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_profile_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p]),
    ("sdt_gpu_profile_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_uint32, _c.c_void_p]),
    ("sdt_gpu_profile_kept_reads", _c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_correct_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_uint32,
                                                _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_correct_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_correct_kept_reads", _c.c_int, [_c.c_void_p, _c.c_uint32, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64), _c.c_void_p,
                                              _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_kept_batches", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_fetch_kept_batch", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_select_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_select_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_int, _c.c_void_p,
                                               _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_select_kept_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64,
                                             _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_compact_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                         _c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_compact_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                                _c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_trim_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                      _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_trim_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                             _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_trim_kept_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64),
                                           _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_compact_trimmed", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                           _c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_compact_trimmed_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                                  _c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_dedup_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_dedup_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_void_p,
                                              _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_dedup_kept_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64,
                                            _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_clip_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                      _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_clip_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                             _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_clip_kept_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64),
                                           _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_overlap_pairs", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                         _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_overlap_pairs_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_overlap_kept_pairs", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64,
                                              _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_complexity_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                            _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_complexity_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                   _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_complexity_kept_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64),
                                                 _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_quality_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_quality_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_screen_load", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint32, _c.c_uint32,
                                       _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_screen_unload", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_screen_info", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_screen_lookup", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_screen_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_screen_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_void_p, _c.c_void_p,
                                               _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_screen_kept_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64,
                                             _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_merge_pairs", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_merge_pairs_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                              _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.POINTER(_c.c_uint64),
                                              _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_merge_kept_pairs", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                            _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64),
                                            _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_compact_quals_trimmed", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                                 _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_compact_quals_trimmed_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                                        _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_qc_report_words", _c.c_uint64, [_c.c_uint32]),
    ("sdt_gpu_qc_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p,
                                    _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64]),
    ("sdt_gpu_qc_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                           _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_asm_begin", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_asm_add", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_asm_add_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_asm_spectrum", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_asm_end", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_compare_tables", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_compare_select", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_cluster_begin", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_cluster_components", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_cluster_lookup", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_cluster_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_uint32, _c.c_uint32,
                                         _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_cluster_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int, _c.c_uint32, _c.c_uint32,
                                                _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_cluster_kept_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint32, _c.c_uint32, _c.c_void_p, _c.c_uint64,
                                              _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_cluster_end", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_bubbles_begin", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_bubbles_fetch", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_bubbles_paths", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_bubbles_end", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_unitigs_begin", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_unitigs_fetch", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_unitigs_seqs", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_unitigs_links", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64), _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_unitigs_end", _c.c_int, [_c.c_void_p]),
    ("sdt_gpu_unitigs_index", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_unitigs_lookup", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_unitigs_reads", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                         _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_unitigs_reads_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64,
                                                _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_unitigs_support_begin", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_unitigs_support_add", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.c_int]),
    ("sdt_gpu_unitigs_support_add_device", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_int]),
    ("sdt_gpu_unitigs_support_unitigs", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p]),
    ("sdt_gpu_unitigs_support_links", _c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_unitigs_support_junctions", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_unitigs_support_mates", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.POINTER(_c.c_uint64)]),
    ("sdt_gpu_unitigs_support_totals", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("sdt_gpu_unitigs_support_end", _c.c_int, [_c.c_void_p]),
]
ABI_SYMBOLS = [n for n, _, _ in _ABI]

# sdt_read_cov (include/sdt_gpu.h): one record per read of a k-mer coverage profile
READ_COV_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "found", "solid", "min", "median", "max")])
COV_TOO_LONG = 0xFFFFFFFF
# sdt_read_fix (include/sdt_gpu.h): one record per read of a correction; an edit is read << 18 | pos << 2 | new_base
READ_FIX_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "weak", "runs", "fixed")])
# sdt_read_pick (include/sdt_gpu.h): one record per read of a normalisation; verdict = class 0..4 | 1 << 4 iff the read itself is aberrant
READ_PICK_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "median", "cov", "verdict")])
PICK_KEPT, PICK_KEPT_DRAW, PICK_DROPPED_DRAW, PICK_ABERRANT, PICK_SHORT = range(5)
PICK_OWN_ABERRANT = 1 << 4
# sdt_read_trim (include/sdt_gpu.h): one record per read of a trim; the kept bases are [start, start + len) of the read
READ_TRIM_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "weak", "median", "start", "len", "verdict")])
TRIM_WHOLE, TRIM_GATED, TRIM_TRIMMED, TRIM_DROPPED, TRIM_SHORT = range(5)
TRIM_CORRECTED = 1                                       # SDT_TRIM_CORRECTED
# sdt_read_dup (include/sdt_gpu.h): one record per read of a duplicate filter; first = the smallest unit id of the read's class
READ_DUP_DTYPE = np.dtype([("first", np.uint64), ("copies", np.uint32), ("verdict", np.uint32)])
DUP_KEPT, DUP_DROPPED = range(2)
SDT_DEDUP_MATE_SWAP = 1
# sdt_read_clip (include/sdt_gpu.h): one record per read of a clip; adapters = (1 + 3' adapter, or 0) | (1 + 5' adapter, or 0) << 16; the
# kept bases are [start, start + len) of the read, where READ_TRIM_DTYPE has them
READ_CLIP_DTYPE = np.dtype([(f, np.uint32) for f in ("adapters", "tail3", "tail5", "start", "len", "verdict")])
CLIP_WHOLE, CLIP_CLIPPED, CLIP_DROPPED = 0, 2, 3
CLIP_MAX_ADAPTERS, CLIP_MAX_ADAPTER_LEN = 256, 128
# sdt_read_overlap (include/sdt_gpu.h): one record per read of a mate overlap; overlap, mismatches and insert are the pair's (0: none); the
# kept bases are [start, start + len) of the read, where READ_TRIM_DTYPE has them
READ_OVERLAP_DTYPE = np.dtype([(f, np.uint32) for f in ("overlap", "mismatches", "insert", "start", "len", "verdict")])
OVERLAP_WHOLE, OVERLAP_CLIPPED, OVERLAP_DROPPED = 0, 2, 3
# sdt_read_complexity (include/sdt_gpu.h): one record per read of a low-complexity filter; windows scored, LOW windows, the highest window
# score in percent; the kept bases are [start, start + len) of the read, where READ_TRIM_DTYPE has them
READ_COMPLEXITY_DTYPE = np.dtype([(f, np.uint32) for f in ("windows", "low", "score", "start", "len", "verdict")])
COMPLEXITY_WHOLE, COMPLEXITY_CLIPPED, COMPLEXITY_DROPPED = 0, 2, 3
SDT_COMPLEXITY_TRIM = 1
# sdt_read_quality (include/sdt_gpu.h): one record per read of a quality trim; the bases of the best segment, those of them below
# low_q, its expected errors per million bases; the kept bases are [start, start + len) of the read, where READ_TRIM_DTYPE has them
READ_QUALITY_DTYPE = np.dtype([(f, np.uint32) for f in ("span", "low", "ee_ppm", "start", "len", "verdict")])
QUALITY_WHOLE, QUALITY_CLIPPED, QUALITY_DROPPED = 0, 2, 3
# sdt_read_screen (include/sdt_gpu.h): one record per read of a reference screen; its k-mers, those of them in the set, the smallest
# reference among them (SCREEN_NO_REF: none); len = the read's bases if kept, else 0, where READ_TRIM_DTYPE has it; verdict 0 kept, 1 dropped
READ_SCREEN_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "hits", "ref", "start", "len", "verdict")])
SCREEN_KEPT, SCREEN_DROPPED = range(2)
SCREEN_KEEP_MATCHED = 1                                  # SDT_SCREEN_KEEP_MATCHED
SCREEN_NO_REF = 0xFFFFFFFF
# sdt_read_merge (include/sdt_gpu.h): one record per read of a merge; merged = the fragment's bases (0: the pair was not merged),
# mismatches = the mismatch columns of the overlap, from_b = those of them decided for mate 2 by the qualities; start, len and verdict
# say what is left of the read in the stream of unmerged reads, where READ_TRIM_DTYPE has them (a merged pair: 0, 0, MERGE_MERGED)
READ_MERGE_DTYPE = np.dtype([(f, np.uint32) for f in ("merged", "mismatches", "from_b", "start", "len", "verdict")])
MERGE_MERGED = 5                                         # SDT_MERGE_MERGED
# the QC report (include/sdt_gpu.h): a flat uint64 array of 203 + 99 (cycles + 1) words that qc_reads ADDS to; qc_sections cuts it up
QC_MAX_CYCLES = 4096                                     # SDT_QC_MAX_CYCLES
QC_FROM_END = 1                                          # SDT_QC_FROM_END
QC_TILE = 152                                            # rows of the kernel's LDS tile (csrc/sdt_read_plan.h: QC_TILE; tools/qc_plan_check.cpp prints it)
QC_QUALS, QC_GC_BINS, QC_TOTALS = 94, 101, 8
# sdt_seq_support (include/sdt_gpu.h): one record of 32 bytes per sequence of an assembly scored against the counted table; sum = the
# sum of its k-mers' counts, a gap = a maximal run of weak k-mers, longest_at = the first k-mer of the longest (kmers: none)
SEQ_SUPPORT_DTYPE = np.dtype([("sum", np.uint64)] + [(f, np.uint32) for f in ("kmers", "found", "solid", "gaps", "longest_gap", "longest_at")])
ASM_CN_COLS, ASM_MAX_ROWS = 8, 1024                      # SDT_ASM_CN_COLS, SDT_ASM_MAX_ROWS
CMP_MAX_CELLS = 16384                                    # SDT_CMP_MAX_CELLS
# sdt_read_cluster (include/sdt_gpu.h): one record per read of a clustering; cluster = the id of its first live k-mer, split = its live
# k-mers in another cluster, unit = the cluster of its unit (a read or a pair); sdt_cluster_comp: one record of 16 bytes per cluster
READ_CLUSTER_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "live", "split", "cluster", "unit", "verdict")])
CLUSTER_COMP_DTYPE = np.dtype([("count_sum", np.uint64), ("nodes", np.uint32), ("reserved", np.uint32)])
CLUSTER_NONE = 0xFFFFFFFF                                # SDT_CLUSTER_NONE
CLUSTER_WHOLE, CLUSTER_NOT_WHOLE, CLUSTER_THROUGH_MATE, CLUSTER_UNASSIGNED, CLUSTER_SHORT = range(5)
# sdt_bubble (include/sdt_gpu.h): one record of 48 bytes per bubble of the counted k-mer graph; info = base_a | base_b << 2 |
# link_a << 8 | link_b << 16
BUBBLE_DTYPE = np.dtype([("sum_a", np.uint64), ("sum_b", np.uint64)] +
                        [(f, np.uint32) for f in ("len_a", "len_b", "min_a", "min_b", "src_count", "snk_count", "info", "reserved")])
BUBBLE_MAX_LEN = 1 << 20                                 # SDT_BUBBLE_MAX_LEN
# sdt_unitig (include/sdt_gpu.h): one record of 24 bytes per unitig of the counted k-mer graph; info = circular | indeg(first word) << 4 |
# outdeg(last word) << 8.  sdt_unitig_link: 16 bytes per link; info = o | o' << 1 | base << 2 | link counter << 8
UNITIG_DTYPE = np.dtype([("sum", np.uint64)] + [(f, np.uint32) for f in ("nodes", "min", "max", "info")])
UNITIG_LINK_DTYPE = np.dtype([(f, np.uint32) for f in ("from", "to", "info", "reserved")])
# reads threaded through the unitig list (include/sdt_gpu.h).  sdt_unitig_pos: the place of a k-mer, info = o of the word as given.
# sdt_read_path: one record of 24 bytes per read.  sdt_path_seg: one of 24 bytes per segment; info = o | join << 1
UNITIG_NONE = 0xFFFFFFFF                                 # SDT_UNITIG_NONE
UNITIG_POS_DTYPE = np.dtype([(f, np.uint32) for f in ("unitig", "pos", "info", "reserved")])
READ_PATH_DTYPE = np.dtype([(f, np.uint32) for f in ("kmers", "live", "segs", "breaks", "first", "last")])
PATH_SEG_DTYPE = np.dtype([(f, np.uint32) for f in ("unitig", "info", "read_pos", "unitig_pos", "kmers", "reserved")])
# read support tallied on the unitig list (include/sdt_gpu.h).  An oriented unitig is unitig << 1 | o.  sdt_unitig_support: 16 bytes per
# unitig; sdt_link_support: 16 per link record of unitigs_links; sdt_unitig_junction: 24 per junction; sdt_mate_link: 16 per mate link
UNITIG_SUPPORT_DTYPE = np.dtype([("segs", np.uint64), ("kmers", np.uint64)])
LINK_SUPPORT_DTYPE = np.dtype([("along", np.uint64), ("against", np.uint64)])
UNITIG_JUNCTION_DTYPE = np.dtype([(f, np.uint32) for f in ("from", "via", "to", "reserved")] + [("count", np.uint64)])
MATE_LINK_DTYPE = np.dtype([("from", np.uint32), ("to", np.uint32), ("pairs", np.uint64)])
SUPPORT_TOTALS = ("reads", "placed", "segments", "live", "traversals", "no_record", "passages", "pairs", "pairs_placed", "pairs_within", "pairs_linked",
                  "dropped")


class NormParams(_c.Structure):
    """sdt_norm_params"""
    _fields_ = [("target", _c.c_uint32), ("max_cv_pct", _c.c_uint32), ("seed", _c.c_uint64)]


class TrimParams(_c.Structure):
    """sdt_trim_params"""
    _fields_ = [("min_count", _c.c_uint32), ("min_cov", _c.c_uint32), ("min_len", _c.c_uint32), ("flags", _c.c_uint32)]


class DedupParams(_c.Structure):
    """sdt_dedup_params"""
    _fields_ = [("flags", _c.c_uint32), ("reserved", _c.c_uint32)]


class ClipParams(_c.Structure):
    """sdt_clip_params; tail3_bases / tail5_bases: masks of base codes (A 1, C 2, T 4, G 8)"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_overlap", "max_err_pct", "min_len", "min_tail", "tail_err_pct", "tail3_bases", "tail5_bases",
                                           "flags")]


class OverlapParams(_c.Structure):
    """sdt_overlap_params; the defaults of `sdt-kmers overlap`"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_overlap", "max_err_pct", "min_len", "flags")]

    def __init__(self, min_overlap=30, max_err_pct=10, min_len=0, flags=0):
        super().__init__(min_overlap, max_err_pct, min_len, flags)


class ComplexityParams(_c.Structure):
    """sdt_complexity_params; the defaults of `sdt-kmers complexity`"""
    _fields_ = [(f, _c.c_uint32) for f in ("max_score_pct", "max_low_pct", "min_len", "flags")]

    def __init__(self, max_score_pct=10, max_low_pct=50, min_len=0, flags=0):
        super().__init__(max_score_pct, max_low_pct, min_len, flags)


class QualityParams(_c.Structure):
    """sdt_quality_params; the defaults of `sdt-kmers qtrim`"""
    _fields_ = [(f, _c.c_uint32) for f in ("phred_offset", "cut_q", "low_q", "max_low_pct", "max_ee_ppm", "min_len", "flags", "reserved")]

    def __init__(self, phred_offset=33, cut_q=20, low_q=15, max_low_pct=40, max_ee_ppm=0, min_len=0, flags=0, reserved=0):
        super().__init__(phred_offset, cut_q, low_q, max_low_pct, max_ee_ppm, min_len, flags, reserved)


class ScreenParams(_c.Structure):
    """sdt_screen_params; the defaults of `sdt-kmers screen`"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_hits", "min_hit_pct", "flags", "reserved")]

    def __init__(self, min_hits=1, min_hit_pct=0, flags=0, reserved=0):
        super().__init__(min_hits, min_hit_pct, flags, reserved)


class MergeParams(_c.Structure):
    """sdt_merge_params; the defaults of `sdt-kmers merge`"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_len", "max_len", "phred_offset", "flags")]

    def __init__(self, min_len=0, max_len=0, phred_offset=33, flags=0):
        super().__init__(min_len, max_len, phred_offset, flags)


class QcParams(_c.Structure):
    """sdt_qc_params; the defaults of `sdt-kmers qc`"""
    _fields_ = [(f, _c.c_uint32) for f in ("cycles", "phred_offset", "flags", "class_sel", "reserved")]

    def __init__(self, cycles=1024, phred_offset=33, flags=0, class_sel=0, reserved=0):
        super().__init__(cycles, phred_offset, flags, class_sel, reserved)


class AsmParams(_c.Structure):
    """sdt_asm_params; the defaults of `sdt-kmers evaluate`"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_count", "rows", "flags", "reserved")]

    def __init__(self, min_count=2, rows=256, flags=0, reserved=0):
        super().__init__(min_count, rows, flags, reserved)


class CmpParams(_c.Structure):
    """sdt_cmp_params; the defaults of `sdt-kmers compare`"""
    _fields_ = [(f, _c.c_uint32) for f in ("rows", "cols", "flags", "reserved")]

    def __init__(self, rows=64, cols=64, flags=0, reserved=0):
        super().__init__(rows, cols, flags, reserved)


class ClusterParams(_c.Structure):
    """sdt_cluster_params; the defaults of `sdt-kmers cluster`"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_count", "max_count", "min_link", "flags")]

    def __init__(self, min_count=2, max_count=0, min_link=1, flags=0):
        super().__init__(min_count, max_count, min_link, flags)


class BubbleParams(_c.Structure):
    """sdt_bubble_params; the defaults of `sdt-kmers bubbles`"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_count", "max_count", "min_link", "max_len", "flags", "reserved")]

    def __init__(self, min_count=2, max_count=0, min_link=1, max_len=1000, flags=0, reserved=0):
        super().__init__(min_count, max_count, min_link, max_len, flags, reserved)


class UnitigParams(_c.Structure):
    """sdt_unitig_params; the defaults of `sdt-kmers unitigs`"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_count", "max_count", "min_link", "flags")]

    def __init__(self, min_count=2, max_count=0, min_link=1, flags=0):
        super().__init__(min_count, max_count, min_link, flags)


class SupportParams(_c.Structure):
    """sdt_support_params; a capacity of 0: that list is not kept"""
    _fields_ = [("junction_capacity", _c.c_uint64), ("mate_capacity", _c.c_uint64), ("flags", _c.c_uint32), ("reserved", _c.c_uint32)]

    def __init__(self, junction_capacity=0, mate_capacity=0, flags=0, reserved=0):
        super().__init__(junction_capacity, mate_capacity, flags, reserved)


class CmpRange(_c.Structure):
    """sdt_cmp_range; the default: the k-mers of A that B does not hold"""
    _fields_ = [(f, _c.c_uint32) for f in ("min_a", "max_a", "min_b", "max_b")]

    def __init__(self, min_a=1, max_a=2**32 - 1, min_b=0, max_b=0):
        super().__init__(min_a, max_a, min_b, max_b)


def qc_report_words(cycles: int) -> int:
    """words of the report for `cycles` cycles: 203 + 99 (cycles + 1); 0 for cycles out of range (sdt_gpu_qc_report_words)"""
    return int(load_library().sdt_gpu_qc_report_words(cycles))


def qc_sections(report: np.ndarray, cycles: int) -> dict:
    """the sections of a report as numpy VIEWS: totals[8], base[R][4], qual[R][94], len[R], gc[101], meanq[94]; R = cycles + 1"""
    R = cycles + 1
    assert report.dtype == np.uint64 and report.ndim == 1 and report.size >= QC_TOTALS + 99 * R + QC_GC_BINS + QC_QUALS
    out, at = {}, 0
    for name, shape in (("totals", (QC_TOTALS,)), ("base", (R, 4)), ("qual", (R, QC_QUALS)), ("len", (R,)), ("gc", (QC_GC_BINS,)),
                        ("meanq", (QC_QUALS,))):
        n = int(np.prod(shape))
        out[name] = report[at: at + n].reshape(shape)
        at += n
    return out


class AdapterSet(_c.Structure):
    """sdt_adapter_set"""
    _fields_ = [("words", _c.c_void_p), ("offsets", _c.c_void_p), ("ends", _c.c_void_p), ("n", _c.c_uint32), ("reserved", _c.c_uint32)]


def pack_adapters(adapters):
    """[(codes, end)] -> (AdapterSet, the arrays it points into: keep them alive)"""
    codes = [np.asarray(a, dtype=np.uint8).reshape(-1) for a, _ in adapters]
    offsets = np.zeros(len(codes) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(a) for a in codes], dtype=np.uint64)
    flat = np.concatenate(codes) if codes else np.zeros(0, dtype=np.uint8)
    flat = np.concatenate([flat, np.zeros(-len(flat) % 16 + 16, dtype=np.uint8)]).astype(np.uint32).reshape(-1, 16)
    words = np.ascontiguousarray((flat << (30 - 2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32))
    ends = np.ascontiguousarray([e for _, e in adapters], dtype=np.uint8)
    aset = AdapterSet(words.ctypes.data, offsets.ctypes.data, ends.ctypes.data if len(ends) else None, len(codes), 0)
    return aset, (words, offsets, ends)

_lib = None


class SdtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsdt_gpu error {code}: {msg}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile csrc/ for gfx950 (hipcc cross-compiles without a GPU). Returns the library path."""
    cmd = ["make", "-C", CSRC_DIR] + (["-B"] if force else [])
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def load_library():
    """dlopen libsdt_gpu.so and bind every ABI symbol. Fails loudly when the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    global LIB_PATH
    LIB_PATH = os.environ.get("SDT_GPU_LIB", LIB_PATH)      # (A/B builds of the library: tools/, profiles/)
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the pregraph hashing path)")
    # One HIP runtime per process: torch bundles its own libamdhip64 (soname libamdhip64.so.7, file name
    # libamdhip64.so).  Loaded first, the dynamic linker resolves our NEEDED libamdhip64.so.7 to it; loaded
    # second, torch would map a second runtime next to /opt/rocm's and fail with hipErrorNoDevice.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in _ABI:
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _ptr(a):
    """host numpy array or torch tensor (host or device) or int -> void*"""
    if a is None:
        return None
    if isinstance(a, int):
        return ctypes.c_void_p(a)
    if isinstance(a, np.ndarray):
        return ctypes.c_void_p(a.ctypes.data)
    return ctypes.c_void_p(a.data_ptr())  # torch tensor


def key_words_for(K: int) -> int:
    return 1 if K <= 31 else (2 if K <= 63 else 4)


def clamp_K(K: int, max_k: int = 127) -> int:
    """call_pregraph's K handling (pregraph.c:38-59): even -> +1, < 13 -> 13, > max -> max."""
    if K % 2 == 0:
        K += 1
    if K < 13:
        K = 13
    elif K > max_k:
        K = max_k
    return K


class PregraphGPU:
    """One device context: mirrors sdt_gpu_* one to one (see include/sdt_gpu.h for the reference
    call sites each method replaces)."""

    def __init__(self, K: int, est_distinct: int = 0, device: int = 0, flags: int = 0):
        self.lib = load_library()
        self.K = K
        self._ctx = ctypes.c_void_p()
        rc = self.lib.sdt_gpu_init(ctypes.byref(self._ctx), device, K, est_distinct, flags)
        self._check(rc)
        self.nw = self.lib.sdt_gpu_key_words(self._ctx)

    def _check(self, rc):
        if rc != SDT_OK:
            raise SdtError(rc, self.lib.sdt_gpu_last_error().decode())

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx.value:
            self.lib.sdt_gpu_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- pass 1
    def reset(self):
        self._check(self.lib.sdt_gpu_reset(self._ctx))

    def push_reads(self, packed_words: np.ndarray, offsets: np.ndarray):
        packed_words = np.ascontiguousarray(packed_words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_push_reads(self._ctx, _ptr(packed_words), packed_words.size,
                                                _ptr(offsets), offsets.size - 1))

    def push_reads_async(self, packed_words: np.ndarray, offsets: np.ndarray) -> int:
        """enqueue only; the arrays must stay alive and untouched until push_wait(ticket) (pinned memory keeps the copy asynchronous)"""
        assert packed_words.dtype == np.uint32 and offsets.dtype == np.uint64 and packed_words.flags.c_contiguous and offsets.flags.c_contiguous
        t = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_push_reads_async(self._ctx, _ptr(packed_words), packed_words.size, _ptr(offsets), offsets.size - 1,
                                                      ctypes.byref(t)))
        return t.value

    def push_reads_fixed_async(self, packed_words: np.ndarray, nreads: int, read_len: int) -> int:
        """a batch of equal-length reads: the offsets are made on the device"""
        assert packed_words.dtype == np.uint32 and packed_words.flags.c_contiguous
        t = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_push_reads_fixed_async(self._ctx, _ptr(packed_words), packed_words.size, nreads, read_len, ctypes.byref(t)))
        return t.value

    def push_wait(self, ticket: int):
        self._check(self.lib.sdt_gpu_push_wait(self._ctx, ticket))

    def hint_total_kmers(self, kmers: int):
        self._check(self.lib.sdt_gpu_hint_total_kmers(self._ctx, kmers))

    def count_reads_device(self, d_words, nwords: int, d_offsets, nreads: int, max_read_len: int):
        self._check(self.lib.sdt_gpu_count_reads_device(self._ctx, _ptr(d_words), nwords, _ptr(d_offsets),
                                                        nreads, max_read_len))

    def finish_count(self):
        k, n = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_finish_count(self._ctx, ctypes.byref(k), ctypes.byref(n)))
        return k.value, n.value

    # -- multi-GPU, bucket sharding (include/sdt_gpu.h): every method below except kmer_owner is COLLECTIVE
    def comm_init(self, comm_id: bytes, rank: int, nranks: int):
        """RCCL communicator; comm_id = new_comm_id() of rank 0, handed to every rank"""
        buf = ctypes.create_string_buffer(bytes(comm_id), 128)
        self._check(self.lib.sdt_gpu_comm_init(self._ctx, buf, rank, nranks))

    def comm_init_shm(self, name: str, rank: int, nranks: int):
        """host shared-memory transport: validation where the ranks share one GPU"""
        self._check(self.lib.sdt_gpu_comm_init_shm(self._ctx, name.encode(), rank, nranks))

    def count_reads_sharded(self, d_words, nwords: int, d_offsets, nreads: int, max_read_len: int):
        self._check(self.lib.sdt_gpu_count_reads_sharded(self._ctx, _ptr(d_words) if nreads else None, nwords,
                                                         _ptr(d_offsets) if nreads else None, nreads, max_read_len))

    def push_reads_sharded(self, words: np.ndarray, offsets: np.ndarray):
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_push_reads_sharded(self._ctx, _ptr(words), words.size, _ptr(offsets), offsets.size - 1))

    def allreduce(self, values) -> np.ndarray:
        v = np.ascontiguousarray(values, dtype=np.int64).copy()
        self._check(self.lib.sdt_gpu_allreduce_i64(self._ctx, _ptr(v), v.size))
        return v

    def shard_ranges(self, nranks: int) -> np.ndarray:
        """first level-1 bucket of every rank (+ the end): cut on the first sharded call"""
        a = np.zeros(nranks + 1, dtype=np.uint32)
        self._check(self.lib.sdt_gpu_shard_ranges(self._ctx, _ptr(a)))
        return a

    def comm_stats(self):
        """(bytes sent, bytes received, milliseconds on the exchange stream, exchanges) of this rank"""
        a, b, n, ms = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
        self._check(self.lib.sdt_gpu_comm_stats(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(ms), ctypes.byref(n)))
        return a.value, b.value, ms.value, n.value

    # -- scans
    def delow(self, d: int) -> int:
        r = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_delow(self._ctx, d, ctypes.byref(r)))
        return r.value

    def mark_and_hist(self):
        hist = np.zeros(257, dtype=np.int64)
        lin = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_mark_and_hist(self._ctx, _ptr(hist), ctypes.byref(lin)))
        return hist, lin.value

    def export_nodes(self, with_first: bool = False):
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_export_nodes(self._ctx, None, None, None, None, None, 0, ctypes.byref(n)))
        m = max(n.value, 1)
        keys = np.zeros((m, self.nw), dtype=np.uint64)
        l_links = np.zeros(m, dtype=np.uint32)
        r_flags = np.zeros(m, dtype=np.uint32)
        count = np.zeros(m, dtype=np.uint32)
        first = np.zeros(m, dtype=np.uint64) if with_first else None
        self._check(self.lib.sdt_gpu_export_nodes(self._ctx, _ptr(keys), _ptr(l_links), _ptr(r_flags),
                                                  _ptr(count), _ptr(first), m, ctypes.byref(n)))
        k = n.value
        if with_first:
            return keys[:k], l_links[:k], r_flags[:k], count[:k], first[:k]
        return keys[:k], l_links[:k], r_flags[:k], count[:k]

    def import_nodes(self, keys, l_links, r_flags, count, first=None):
        """nodes as export_nodes gives them (keys distinct, canonical and not in the table yet) into this context's table"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.nw)
        l_links, r_flags, count = (np.ascontiguousarray(a, dtype=np.uint32) for a in (l_links, r_flags, count))
        assert len(l_links) == len(r_flags) == len(count) == len(keys)
        first = None if first is None else np.ascontiguousarray(first, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_import_nodes(self._ctx, _ptr(keys), _ptr(l_links), _ptr(r_flags), _ptr(count), _ptr(first), len(keys)))

    # -- graph-cleaning dry runs on the device mirror (cutTipPreGraph.c)
    def set_node_index(self, keys: np.ndarray):
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.nw)
        self._nidx = len(keys)
        self._check(self.lib.sdt_gpu_set_node_index(self._ctx, _ptr(keys), len(keys)))

    def update_nodes(self, keys, l_links, r_flags):
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.nw)
        l_links = np.ascontiguousarray(l_links, dtype=np.uint32)
        r_flags = np.ascontiguousarray(r_flags, dtype=np.uint32)
        assert len(l_links) == len(keys) == len(r_flags)
        self._check(self.lib.sdt_gpu_update_nodes(self._ctx, _ptr(keys), _ptr(l_links), _ptr(r_flags), len(keys)))

    def tip_walks(self, thin: bool, cut_len: int):
        n = self._nidx
        end = np.zeros(max(n, 1), dtype=np.uint64)
        info = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.lib.sdt_gpu_tip_walks(self._ctx, int(thin), cut_len, _ptr(end), _ptr(info), n))
        return end[:n], info[:n]

    def minor_out_dry(self, threshold: float):
        """-> (records uint64[n, 9], n_junctions): see sdt_gpu_minor_out_dry"""
        cap = max(self._nidx // 8, 1024)
        while True:
            rec = np.zeros((cap, 9), dtype=np.uint64)
            nj, nr = ctypes.c_uint64(), ctypes.c_uint64()
            rc = self.lib.sdt_gpu_minor_out_dry(self._ctx, ctypes.c_double(threshold), _ptr(rec), cap, ctypes.byref(nj), ctypes.byref(nr))
            if rc == SDT_EFULL and nr.value > cap:
                cap = nr.value
                continue
            self._check(rc)
            return rec[: nr.value], nj.value

    def edge_ports(self):
        """-> records uint64[n, 17]: see sdt_gpu_edge_ports"""
        cap = max(self._nidx // 4, 1024)
        while True:
            rec = np.zeros((cap, 17), dtype=np.uint64)
            nr = ctypes.c_uint64()
            rc = self.lib.sdt_gpu_edge_ports(self._ctx, _ptr(rec), cap, ctypes.byref(nr))
            if rc == SDT_EFULL and nr.value > cap:
                cap = nr.value
                continue
            self._check(rc)
            return rec[: nr.value]

    # -- map stage (prlContig2nodes / prlRead2Ctg); the context must be created with FLAG_CONTIG_INDEX
    def index_contigs(self, packed_words: np.ndarray, offsets: np.ndarray, ids: np.ndarray):
        packed_words = np.ascontiguousarray(packed_words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        assert len(ids) == len(offsets) - 1
        self._check(self.lib.sdt_gpu_index_contigs(self._ctx, _ptr(packed_words), packed_words.size, _ptr(offsets),
                                                   _ptr(ids), len(ids)))

    def set_contig_table(self, length: np.ndarray, twin: np.ndarray):
        length = np.ascontiguousarray(length, dtype=np.uint32)
        twin = np.ascontiguousarray(twin, dtype=np.uint32)
        assert len(length) == len(twin)
        self._check(self.lib.sdt_gpu_set_contig_table(self._ctx, _ptr(length), _ptr(twin), len(length) - 1))

    def align_reads(self, packed_words, offsets, align_len=None, align_len_all: int = 0, max_hits=None):
        """-> (read_info uint64[nreads], hits uint32[nhits, 4]); hits[r] = first hit of read r, further hits in the tail;
        see include/sdt_gpu.h for the bit layout"""
        packed_words = np.ascontiguousarray(packed_words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if align_len is not None:
            align_len = np.ascontiguousarray(align_len, dtype=np.int32)
            assert len(align_len) == n
        info = np.zeros(max(n, 1), dtype=np.uint64)
        cap = max_hits if max_hits is not None else 2 * n + 16
        while True:
            hits = np.zeros((max(cap, 1), 4), dtype=np.uint32)
            got = ctypes.c_uint64()
            rc = self.lib.sdt_gpu_align_reads(self._ctx, _ptr(packed_words), packed_words.size, _ptr(offsets), n,
                                              _ptr(align_len), align_len_all, _ptr(info), _ptr(hits), cap, ctypes.byref(got))
            if rc == SDT_EFULL and max_hits is None and got.value > cap:      # SDT_EFULL: the hit array was too small
                cap = got.value
                continue
            self._check(rc)
            return info[:n], hits[: got.value]

    def tip_walks_compact(self, thin: bool, cut_len: int):
        """-> records uint64[n, 2]: node index | info << 56, end index"""
        cap = max(self._nidx // 8, 1024)
        while True:
            rec = np.zeros((cap, 2), dtype=np.uint64)
            nr = ctypes.c_uint64()
            rc = self.lib.sdt_gpu_tip_walks_compact(self._ctx, int(thin), cut_len, _ptr(rec), cap, ctypes.byref(nr))
            if rc == SDT_EFULL and nr.value > cap:
                cap = nr.value
                continue
            self._check(rc)
            return rec[: nr.value]

    # -- the reference's visiting order on the device, labelled dry runs (include/sdt_gpu.h)
    def layout_sorted_keys(self, p: int, nw_variant: int):
        """-> (keys uint64[n, nw] sorted by (set, first occurrence), set_start uint64[p + 1])"""
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_layout_sorted_keys(self._ctx, p, nw_variant, None, 0, None, ctypes.byref(n)))
        keys = np.zeros((max(n.value, 1), self.nw), dtype=np.uint64)
        ss = np.zeros(p + 1, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_layout_sorted_keys(self._ctx, p, nw_variant, _ptr(keys), n.value, _ptr(ss), ctypes.byref(n)))
        return keys[: n.value], ss

    def layout_on_device(self, p: int, nw_variant: int, small_init: bool = False):
        """sort + replay of the probing + numbering, all on the device -> set_start uint64[p + 1]"""
        ss = np.zeros(p + 1, dtype=np.uint64)
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_layout_on_device(self._ctx, p, nw_variant, int(small_init), _ptr(ss), ctypes.byref(n)))
        self._nidx = n.value
        return ss

    def layout_apply(self, order: np.ndarray):
        order = np.ascontiguousarray(order, dtype=np.uint64)
        self._nidx = len(order)
        self._check(self.lib.sdt_gpu_layout_apply(self._ctx, _ptr(order), len(order)))

    def export_ordered(self):
        n = self._nidx
        keys = np.zeros((max(n, 1), self.nw), dtype=np.uint64)
        l, r, cnt = (np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3))
        self._check(self.lib.sdt_gpu_export_ordered(self._ctx, _ptr(keys), _ptr(l), _ptr(r), _ptr(cnt), n))
        return keys[:n], l[:n], r[:n], cnt[:n]

    def update_nodes_by_index(self, node, l_links, r_flags):
        node = np.ascontiguousarray(node, dtype=np.uint64)
        l_links = np.ascontiguousarray(l_links, dtype=np.uint32)
        r_flags = np.ascontiguousarray(r_flags, dtype=np.uint32)
        assert len(l_links) == len(node) == len(r_flags)
        self._check(self.lib.sdt_gpu_update_nodes_by_index(self._ctx, _ptr(node), _ptr(l_links), _ptr(r_flags), len(node)))

    def _fetch(self, n: int, words: int):
        rec = np.zeros((max(n, 1), words), dtype=np.uint64)
        self._check(self.lib.sdt_gpu_fetch_records(self._ctx, _ptr(rec), n * words))
        return rec[:n]

    def tip_walks_labelled(self, thin: bool, cut_len: int):
        """-> records uint64[n, 3]: node index | info << 56, end index, component label; sorted by (label, node)"""
        nr = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_tip_walks_labelled(self._ctx, int(thin), cut_len, ctypes.byref(nr)))
        return self._fetch(nr.value, 3)

    def minor_out_labelled(self, threshold: float):
        """-> (records uint64[n, 14], n_junctions): node, 8 neighbours, 8 counts (two per word), label; the junction records sorted by (label, node)"""
        nj, nr = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_minor_out_labelled(self._ctx, ctypes.c_double(threshold), ctypes.byref(nj), ctypes.byref(nr)))
        return self._fetch(nr.value, 14), nj.value

    def minor_out_commit(self, threshold: float, max_component: int = 1 << 62):
        """removeMinorOut's commit on the device: labelled dry run + commit.  -> dict(records, n_junctions, largest, off, linear,
        node, l_links, r_flags, skipped, skipped_neighbours): the records of the dry run, the nodes the commit wrote, the junction
        records of the components it left to the caller and the records of the neighbours those may cut"""
        nj, nr = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_minor_out_labelled(self._ctx, ctypes.c_double(threshold), ctypes.byref(nj), ctypes.byref(nr)))
        big, off, lin, nw, nsk, nskr = (ctypes.c_uint64() for _ in range(6))
        self._check(self.lib.sdt_gpu_minor_out_commit(self._ctx, ctypes.c_double(threshold), max_component, ctypes.byref(big), ctypes.byref(off),
                                                      ctypes.byref(lin), ctypes.byref(nw), ctypes.byref(nsk), ctypes.byref(nskr)))
        node = np.zeros(max(nw.value, 1), dtype=np.uint64)
        l = np.zeros(max(nw.value, 1), dtype=np.uint32)
        r = np.zeros(max(nw.value, 1), dtype=np.uint32)
        self._check(self.lib.sdt_gpu_fetch_written(self._ctx, _ptr(node), _ptr(l), _ptr(r), nw.value))
        sk = np.zeros((max(nskr.value, 1), 14), dtype=np.uint64)
        self._check(self.lib.sdt_gpu_fetch_skipped(self._ctx, _ptr(sk), nskr.value))
        rec = self._fetch(nr.value, 14)
        return dict(records=rec, n_junctions=nj.value, largest=big.value, off=off.value, linear=lin.value,
                    node=node[:nw.value], l_links=l[:nw.value], r_flags=r[:nw.value], skipped=sk[:nsk.value], skipped_neighbours=sk[nsk.value:nskr.value])

    def build_edges(self):
        """-> (records uint64[n_edges, 4 + 2 nw], bases bytes, num_ed): see sdt_gpu_build_edges"""
        ne, ids, nb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_build_edges(self._ctx, ctypes.byref(ne), ctypes.byref(ids), ctypes.byref(nb)))
        rec = self._fetch(ne.value, 4 + 2 * self.nw)
        buf = np.zeros(max(nb.value, 1), dtype=np.uint8)
        self._check(self.lib.sdt_gpu_fetch_edge_bases(self._ctx, _ptr(buf), nb.value))
        return rec, buf[: nb.value].tobytes(), ids.value

    # -- read-only questions to the counted table (search_kmerset, newhash.c:239-283)
    def search_kmers(self, keys):
        """keys uint64[n, nw], either strand -> (count, l_links, r_flags uint32[n], status uint8[n]: bit 0 found, bit 1 stored as
        the reverse complement of the query); the words are the stored node's, as export_nodes gives them"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.nw)
        n = len(keys)
        count, l_links, r_flags = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        status = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.sdt_gpu_search_kmers(self._ctx, _ptr(keys), n, _ptr(count), _ptr(l_links), _ptr(r_flags), _ptr(status)))
        return count, l_links, r_flags, status

    def search_kmers_device(self, d_keys, n: int, d_count=None, d_l_links=None, d_r_flags=None, d_status=None):
        """device buffers (torch tensors or addresses); asynchronous on the context's stream"""
        self._check(self.lib.sdt_gpu_search_kmers_device(self._ctx, _ptr(d_keys), n, _ptr(d_count), _ptr(d_l_links), _ptr(d_r_flags), _ptr(d_status)))

    def profile_reads(self, words, offsets, min_count: int = 0) -> np.ndarray:
        """-> READ_COV_DTYPE[nreads]: kmers, found, solid (count >= min_count), min, median (lower), max of every read's k-mer counts"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros(n, dtype=READ_COV_DTYPE)
        self._check(self.lib.sdt_gpu_profile_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, min_count, _ptr(out)))
        return out

    def profile_reads_device(self, d_words, d_offsets, nreads: int, max_read_len: int, min_count: int, d_out):
        """device buffers; d_out holds nreads records of 24 bytes"""
        self._check(self.lib.sdt_gpu_profile_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, max_read_len, min_count, _ptr(d_out)))

    def profile_kept_reads(self, total_reads: int, min_count: int = 0, out: np.ndarray = None):
        """the reads kept in HBM, indexed by read ordinal -> (READ_COV_DTYPE[total_reads], reads profiled)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_COV_DTYPE)
        assert out.dtype == READ_COV_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_profile_kept_reads(self._ctx, min_count, _ptr(out), total_reads, ctypes.byref(n)))
        return out, n.value

    # -- substitution errors corrected against the counted table (the rule: include/sdt_gpu.h)
    def correct_reads(self, words, offsets, min_count: int = 2):
        """-> (READ_FIX_DTYPE[nreads]: kmers, weak, runs, fixed; the packed stream with the substitutions made; the edits uint64[],
        read << 18 | pos << 2 | new_base, ascending)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        fix = np.zeros(n, dtype=READ_FIX_DTYPE)
        out_words = words.copy()
        cap = max(n // 4, 1024)
        while True:
            edits = np.zeros(cap, dtype=np.uint64)
            got = ctypes.c_uint64()
            rc = self.lib.sdt_gpu_correct_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, min_count, _ptr(fix), _ptr(out_words),
                                                _ptr(edits), cap, ctypes.byref(got))
            if rc == SDT_EFULL and got.value > cap:
                cap = got.value
                continue
            self._check(rc)
            return fix, out_words, edits[: got.value]

    def correct_reads_device(self, d_words, nwords: int, d_offsets, nreads: int, max_read_len: int, min_count: int, d_fix,
                             d_out_words=None, d_edits=None, max_edits: int = 0) -> int:
        """device buffers; d_fix holds nreads records of 16 bytes, d_out_words (optional) nwords words, d_edits (optional) max_edits
        words in no particular order -> the number of edits (SdtError SDT_EFULL past max_edits: e.needed says how many)"""
        got = ctypes.c_uint64()
        rc = self.lib.sdt_gpu_correct_reads_device(self._ctx, _ptr(d_words), nwords, _ptr(d_offsets), nreads, max_read_len, min_count,
                                                   _ptr(d_fix), _ptr(d_out_words), _ptr(d_edits), max_edits, ctypes.byref(got))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = got.value
            raise e
        return got.value

    def correct_kept_reads(self, total_reads: int, min_count: int = 2, out: np.ndarray = None):
        """the reads kept in HBM -> (READ_FIX_DTYPE[total_reads] by read ordinal, reads corrected, edits with the ordinal as `read`);
        the kept reads themselves stay as they are: fetch_kept_batch + the edits give the corrected stream"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_FIX_DTYPE)
        assert out.dtype == READ_FIX_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        cap = max(total_reads // 4, 1024)
        while True:
            edits = np.zeros(cap, dtype=np.uint64)
            n, got = ctypes.c_uint64(), ctypes.c_uint64()
            rc = self.lib.sdt_gpu_correct_kept_reads(self._ctx, min_count, _ptr(out), total_reads, ctypes.byref(n), _ptr(edits), cap,
                                                     ctypes.byref(got))
            if rc == SDT_EFULL and got.value > cap:          # (an ordinal past total_reads is SDT_EFULL too, with no edits counted)
                cap = got.value
                continue
            self._check(rc)
            return out, n.value, edits[: got.value]

    def kept_batches(self) -> int:
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_kept_batches(self._ctx, ctypes.byref(n)))
        return n.value

    def fetch_kept_batch(self, i: int):
        """-> (words uint32[nwords], offsets uint64[nreads + 1], ord_base, ord_stride) of kept batch i, as it was pushed"""
        info = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_fetch_kept_batch(self._ctx, i, _ptr(info), None, 0, None, 0))
        words = np.zeros(int(info[0]), dtype=np.uint32)
        offsets = np.zeros(int(info[1]) + 1, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_fetch_kept_batch(self._ctx, i, _ptr(info), _ptr(words), words.size, _ptr(offsets), offsets.size))
        return words, offsets, int(info[2]), int(info[3])

    # -- in-silico normalisation against the counted table (the rule: include/sdt_gpu.h)
    def select_reads(self, words, offsets, target: int = 50, max_cv_pct: int = 10000, seed: int = 0, paired: bool = False):
        """-> (READ_PICK_DTYPE[nreads]: kmers, median, cov, verdict; keep uint8[nreads]; reads kept)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        pick = np.zeros(n, dtype=READ_PICK_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm = NormParams(target, max_cv_pct, seed)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_select_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, int(bool(paired)), ctypes.addressof(prm),
                                                  _ptr(pick), _ptr(keep), ctypes.byref(kept)))
        return pick, keep, kept.value

    def select_reads_device(self, d_words, d_offsets, nreads: int, max_read_len: int, d_pick, d_keep=None, target: int = 50,
                            max_cv_pct: int = 10000, seed: int = 0, paired: bool = False) -> int:
        """device buffers; d_pick holds nreads records of 16 bytes, d_keep (optional) nreads bytes -> reads kept (waits for the kernels)"""
        prm = NormParams(target, max_cv_pct, seed)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_select_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, max_read_len, int(bool(paired)),
                                                         ctypes.addressof(prm), _ptr(d_pick), _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    def select_kept_reads(self, total_reads: int, pair_ranges=(), target: int = 50, max_cv_pct: int = 10000, seed: int = 0,
                          out: np.ndarray = None):
        """the reads kept in HBM; pair_ranges: [first, end) of ordinals that hold interleaved pairs, flat or as rows
        -> (READ_PICK_DTYPE[total_reads] by read ordinal, reads decided, reads kept)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_PICK_DTYPE)
        assert out.dtype == READ_PICK_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        ranges = np.ascontiguousarray(np.asarray(pair_ranges, dtype=np.uint64).reshape(-1))
        assert ranges.size % 2 == 0
        prm = NormParams(target, max_cv_pct, seed)
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_select_kept_reads(self._ctx, ctypes.addressof(prm), _ptr(ranges) if ranges.size else None, ranges.size // 2,
                                                       _ptr(out), total_reads, ctypes.byref(n), ctypes.byref(kept)))
        return out, n.value, kept.value

    def compact_reads(self, words, offsets, keep, out_words_cap: int = None):
        """the reads with keep[i] != 0, packed again -> (words uint32[n_out_words + 4], offsets uint64[n_out_reads + 1]);
        out_words_cap: the room to offer (SdtError SDT_EFULL when it is too small: e.needed says how many words without the pad)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        n = len(offsets) - 1
        assert len(keep) == n
        cap = words.size + 4 if out_words_cap is None else out_words_cap
        out_words = np.full(max(cap, 1), 0xABABABAB, dtype=np.uint32)
        out_offsets = np.zeros(n + 1, dtype=np.uint64)
        nr, nw = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.sdt_gpu_compact_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, _ptr(keep), _ptr(out_words), cap,
                                            _ptr(out_offsets), ctypes.byref(nr), ctypes.byref(nw))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = nw.value
            raise e
        return out_words[: nw.value + 4], out_offsets[: nr.value + 1]

    def compact_reads_device(self, d_words, d_offsets, nreads: int, d_keep, d_out_words, out_words_cap: int, d_out_offsets):
        """device buffers; d_out_offsets holds nreads + 1 words -> (reads kept, words without the 4 pad words); what
        count_reads_device of another context takes.  SdtError SDT_EFULL: e.needed = the words without the pad"""
        nr, nw = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.sdt_gpu_compact_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, _ptr(d_keep), _ptr(d_out_words),
                                                   out_words_cap, _ptr(d_out_offsets), ctypes.byref(nr), ctypes.byref(nw))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = nw.value
            raise e
        return nr.value, nw.value

    # -- reads trimmed to their longest solid stretch against the counted table (the rule: include/sdt_gpu.h)
    def trim_reads(self, words, offsets, min_count: int = 2, min_cov: int = 0, min_len: int = 0, flags: int = 0):
        """-> (READ_TRIM_DTYPE[nreads]: kmers, weak, median, start, len, verdict; keep uint8[nreads]; reads with len > 0)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        trim = np.zeros(n, dtype=READ_TRIM_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm = TrimParams(min_count, min_cov, min_len, flags)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_trim_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, ctypes.addressof(prm), _ptr(trim), _ptr(keep),
                                                ctypes.byref(kept)))
        return trim, keep, kept.value

    def trim_reads_device(self, d_words, d_offsets, nreads: int, max_read_len: int, d_trim, d_keep=None, min_count: int = 2, min_cov: int = 0,
                          min_len: int = 0, flags: int = 0) -> int:
        """device buffers; d_trim holds nreads records of 24 bytes, d_keep (optional) nreads bytes -> reads with len > 0 (waits for the kernel)"""
        prm = TrimParams(min_count, min_cov, min_len, flags)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_trim_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, max_read_len, ctypes.addressof(prm),
                                                       _ptr(d_trim), _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    def trim_kept_reads(self, total_reads: int, min_count: int = 2, min_cov: int = 0, min_len: int = 0, flags: int = 0, out: np.ndarray = None):
        """the reads kept in HBM -> (READ_TRIM_DTYPE[total_reads] by read ordinal, reads trimmed, reads with len > 0)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_TRIM_DTYPE)
        assert out.dtype == READ_TRIM_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        prm = TrimParams(min_count, min_cov, min_len, flags)
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_trim_kept_reads(self._ctx, ctypes.addressof(prm), _ptr(out), total_reads, ctypes.byref(n), ctypes.byref(kept)))
        return out, n.value, kept.value

    def compact_trimmed(self, words, offsets, trim, out_words_cap: int = None):
        """bases [start, start + len) of every read with len > 0, packed again -> (words uint32[n_out_words + 4], offsets
        uint64[n_out_reads + 1]); out_words_cap: the room to offer (SdtError SDT_EFULL when it is too small: e.needed says how many
        words without the pad)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        trim = np.ascontiguousarray(trim, dtype=READ_TRIM_DTYPE)
        n = len(offsets) - 1
        assert len(trim) == n
        cap = words.size + 4 if out_words_cap is None else out_words_cap
        out_words = np.full(max(cap, 1), 0xABABABAB, dtype=np.uint32)
        out_offsets = np.zeros(n + 1, dtype=np.uint64)
        nr, nw = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.sdt_gpu_compact_trimmed(self._ctx, _ptr(words), words.size, _ptr(offsets), n, _ptr(trim), _ptr(out_words), cap,
                                              _ptr(out_offsets), ctypes.byref(nr), ctypes.byref(nw))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = nw.value
            raise e
        return out_words[: nw.value + 4], out_offsets[: nr.value + 1]

    def compact_trimmed_device(self, d_words, d_offsets, nreads: int, d_trim, d_out_words, out_words_cap: int, d_out_offsets):
        """device buffers; d_out_offsets holds nreads + 1 words -> (reads with len > 0, words without the 4 pad words); what
        count_reads_device of another context takes.  SdtError SDT_EFULL: e.needed = the words without the pad"""
        nr, nw = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.sdt_gpu_compact_trimmed_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, _ptr(d_trim), _ptr(d_out_words),
                                                     out_words_cap, _ptr(d_out_offsets), ctypes.byref(nr), ctypes.byref(nw))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = nw.value
            raise e
        return nr.value, nw.value

    # -- exact copies of a read or of a read pair dropped; needs no counted table (the rule: include/sdt_gpu.h)
    def dedup_reads(self, words, offsets, paired: bool = False, flags: int = 0):
        """-> (READ_DUP_DTYPE[nreads]: first, copies, verdict; keep uint8[nreads]; reads kept)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        dup = np.zeros(n, dtype=READ_DUP_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm = DedupParams(flags, 0)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_dedup_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, int(bool(paired)), ctypes.addressof(prm),
                                                 _ptr(dup), _ptr(keep), ctypes.byref(kept)))
        return dup, keep, kept.value

    def dedup_reads_device(self, d_words, d_offsets, nreads: int, d_dup, d_keep=None, paired: bool = False, flags: int = 0) -> int:
        """device buffers; d_dup holds nreads records of 16 bytes, d_keep (optional) nreads bytes -> reads kept (waits for the kernels)"""
        prm = DedupParams(flags, 0)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_dedup_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, int(bool(paired)),
                                                        ctypes.addressof(prm), _ptr(d_dup), _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    def dedup_kept_reads(self, total_reads: int, pair_ranges=(), flags: int = 0, out: np.ndarray = None):
        """the reads kept in HBM; pair_ranges: [first, end) of ordinals that hold interleaved pairs, flat or as rows
        -> (READ_DUP_DTYPE[total_reads] by read ordinal, reads decided, reads kept)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_DUP_DTYPE)
        assert out.dtype == READ_DUP_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        ranges = np.ascontiguousarray(np.asarray(pair_ranges, dtype=np.uint64).reshape(-1))
        assert ranges.size % 2 == 0
        prm = DedupParams(flags, 0)
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_dedup_kept_reads(self._ctx, ctypes.addressof(prm), _ptr(ranges) if ranges.size else None, ranges.size // 2,
                                                      _ptr(out), total_reads, ctypes.byref(n), ctypes.byref(kept)))
        return out, n.value, kept.value

    # -- adapters and poly-A/T tails clipped from reads; needs no counted table (the rule: include/sdt_gpu.h)
    @staticmethod
    def _clip_args(adapters, params):
        """adapters: [(codes, end)] (end 0: 3', 1: 5') or a ready (AdapterSet, arrays); params: ClipParams or its fields as a dict"""
        prm = params if isinstance(params, ClipParams) else ClipParams(**(params or {}))
        aset, alive = adapters if adapters and isinstance(adapters[0], AdapterSet) else pack_adapters(list(adapters or ()))
        return prm, aset, alive

    def clip_reads(self, words, offsets, adapters=(), params=None):
        """-> (READ_CLIP_DTYPE[nreads]: adapters, tail3, tail5, start, len, verdict; keep uint8[nreads]; reads with len > 0)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        clip = np.zeros(n, dtype=READ_CLIP_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm, aset, alive = self._clip_args(adapters, params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_clip_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, ctypes.addressof(prm), ctypes.addressof(aset),
                                                _ptr(clip), _ptr(keep), ctypes.byref(kept)))
        return clip, keep, kept.value

    def clip_reads_device(self, d_words, d_offsets, nreads: int, d_clip, d_keep=None, adapters=(), params=None) -> int:
        """device buffers; d_clip holds nreads records of 24 bytes (what compact_trimmed_device takes), d_keep (optional) nreads bytes
        -> reads with len > 0 (waits for the kernel)"""
        prm, aset, alive = self._clip_args(adapters, params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_clip_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, ctypes.addressof(prm),
                                                       ctypes.addressof(aset), _ptr(d_clip), _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    def clip_kept_reads(self, total_reads: int, adapters=(), params=None, out: np.ndarray = None):
        """the reads kept in HBM -> (READ_CLIP_DTYPE[total_reads] by read ordinal, reads clipped, reads with len > 0)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_CLIP_DTYPE)
        assert out.dtype == READ_CLIP_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        prm, aset, alive = self._clip_args(adapters, params)
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_clip_kept_reads(self._ctx, ctypes.addressof(prm), ctypes.addressof(aset), _ptr(out), total_reads,
                                                     ctypes.byref(n), ctypes.byref(kept)))
        return out, n.value, kept.value

    # -- the overlap of the two mates of a pair; read-through pairs clipped without an adapter list (the rule: include/sdt_gpu.h)
    @staticmethod
    def _overlap_params(params):
        """params: OverlapParams or its fields as a dict"""
        return params if isinstance(params, OverlapParams) else OverlapParams(**(params or {}))

    def overlap_pairs(self, words, offsets, params=None):
        """reads 2t and 2t + 1 are mates
        -> (READ_OVERLAP_DTYPE[nreads]: overlap, mismatches, insert, start, len, verdict; keep uint8[nreads]; reads with len > 0)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        ov = np.zeros(n, dtype=READ_OVERLAP_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm = self._overlap_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_overlap_pairs(self._ctx, _ptr(words), words.size, _ptr(offsets), n, ctypes.addressof(prm), _ptr(ov), _ptr(keep),
                                                   ctypes.byref(kept)))
        return ov, keep, kept.value

    def overlap_pairs_device(self, d_words, d_offsets, nreads: int, d_ov, d_keep=None, params=None) -> int:
        """device buffers; d_ov holds nreads records of 24 bytes (what compact_trimmed_device takes), d_keep (optional) nreads bytes
        -> reads with len > 0 (waits for the kernel)"""
        prm = self._overlap_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_overlap_pairs_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, ctypes.addressof(prm), _ptr(d_ov),
                                                          _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    def overlap_kept_pairs(self, total_reads: int, pair_ranges=(), params=None, out: np.ndarray = None):
        """the reads kept in HBM; pair_ranges: [first, end) of ordinals that hold interleaved pairs, flat or as rows
        -> (READ_OVERLAP_DTYPE[total_reads] by read ordinal, reads decided, reads with len > 0)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_OVERLAP_DTYPE)
        assert out.dtype == READ_OVERLAP_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        ranges = np.ascontiguousarray(np.asarray(pair_ranges, dtype=np.uint64).reshape(-1))
        assert ranges.size % 2 == 0
        prm = self._overlap_params(params)
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_overlap_kept_pairs(self._ctx, ctypes.addressof(prm), _ptr(ranges) if ranges.size else None, ranges.size // 2,
                                                        _ptr(out), total_reads, ctypes.byref(n), ctypes.byref(kept)))
        return out, n.value, kept.value

    # -- low-complexity reads flagged, dropped or trimmed; needs no counted table (the rule: include/sdt_gpu.h)
    @staticmethod
    def _complexity_params(params):
        """params: ComplexityParams or its fields as a dict"""
        return params if isinstance(params, ComplexityParams) else ComplexityParams(**(params or {}))

    def complexity_reads(self, words, offsets, params=None):
        """-> (READ_COMPLEXITY_DTYPE[nreads]: windows, low, score, start, len, verdict; keep uint8[nreads]; reads with len > 0)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        cx = np.zeros(n, dtype=READ_COMPLEXITY_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm = self._complexity_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_complexity_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, ctypes.addressof(prm), _ptr(cx),
                                                      _ptr(keep), ctypes.byref(kept)))
        return cx, keep, kept.value

    def complexity_reads_device(self, d_words, d_offsets, nreads: int, d_cx, d_keep=None, params=None) -> int:
        """device buffers; d_cx holds nreads records of 24 bytes (what compact_trimmed_device takes), d_keep (optional) nreads bytes
        -> reads with len > 0 (waits for the kernel)"""
        prm = self._complexity_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_complexity_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, ctypes.addressof(prm), _ptr(d_cx),
                                                             _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    def complexity_kept_reads(self, total_reads: int, params=None, out: np.ndarray = None):
        """the reads kept in HBM -> (READ_COMPLEXITY_DTYPE[total_reads] by read ordinal, reads decided, reads with len > 0)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_COMPLEXITY_DTYPE)
        assert out.dtype == READ_COMPLEXITY_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        prm = self._complexity_params(params)
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_complexity_kept_reads(self._ctx, ctypes.addressof(prm), _ptr(out), total_reads, ctypes.byref(n),
                                                           ctypes.byref(kept)))
        return out, n.value, kept.value

    # -- reads trimmed and filtered by their base qualities; needs no counted table and not the bases (the rule: include/sdt_gpu.h)
    @staticmethod
    def _quality_params(params):
        """params: QualityParams or its fields as a dict"""
        return params if isinstance(params, QualityParams) else QualityParams(**(params or {}))

    def quality_reads(self, quals, offsets, params=None):
        """quals: one byte per base under offsets -> (READ_QUALITY_DTYPE[nreads]: span, low, ee_ppm, start, len, verdict;
        keep uint8[nreads]; reads with len > 0)"""
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros(n, dtype=READ_QUALITY_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm = self._quality_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_quality_reads(self._ctx, _ptr(quals), quals.size, _ptr(offsets), n, ctypes.addressof(prm), _ptr(out),
                                                   _ptr(keep), ctypes.byref(kept)))
        return out, keep, kept.value

    def quality_reads_device(self, d_quals, d_offsets, nreads: int, d_out, d_keep=None, params=None) -> int:
        """device buffers; d_quals 4-byte aligned, d_out holds nreads records of 24 bytes (what compact_trimmed_device takes), d_keep
        (optional) nreads bytes -> reads with len > 0 (waits for the kernel)"""
        prm = self._quality_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_quality_reads_device(self._ctx, _ptr(d_quals), _ptr(d_offsets), nreads, ctypes.addressof(prm), _ptr(d_out),
                                                          _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    # -- the per-cycle QC report of a batch: histograms that the call ADDS to; needs no counted table (the rule: include/sdt_gpu.h)
    @staticmethod
    def _qc_params(params):
        """params: QcParams or its fields as a dict"""
        return params if isinstance(params, QcParams) else QcParams(**(params or {}))

    def qc_reads(self, words, offsets, quals=None, ranges=None, classes=None, params=None, report: np.ndarray = None, nbytes: int = None):
        """a host batch; quals (optional) one byte per base under offsets, ranges (optional) 24-byte records with start and len where
        READ_TRIM_DTYPE has them, classes (optional) uint8[nreads] -> the report (uint64), which the call ADDS to (a new one is zero)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        prm = self._qc_params(params)
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
        if ranges is not None:
            ranges = np.ascontiguousarray(ranges)
            assert ranges.dtype.itemsize == 24 and len(ranges) == n
        if classes is not None:
            classes = np.ascontiguousarray(classes, dtype=np.uint8)
            assert len(classes) == n
        if report is None:
            report = np.zeros(max(qc_report_words(prm.cycles), 1), dtype=np.uint64)
        assert report.dtype == np.uint64 and report.flags.c_contiguous
        nb = (quals.size if quals is not None else 0) if nbytes is None else nbytes
        self._check(self.lib.sdt_gpu_qc_reads(self._ctx, _ptr(words), words.size, _ptr(quals), nb, _ptr(offsets), n, _ptr(ranges), _ptr(classes),
                                              ctypes.addressof(prm), _ptr(report), report.size))
        return report

    def qc_reads_device(self, d_words, d_offsets, nreads: int, d_report, d_quals=None, d_ranges=None, d_classes=None, params=None):
        """device buffers; d_quals (optional) 4-byte aligned, d_ranges (optional) nreads records of 24 bytes, d_classes (optional) nreads
        bytes, d_report 8-byte aligned uint64 words that the call ADDS to (waits for the kernel)"""
        prm = self._qc_params(params)
        self._check(self.lib.sdt_gpu_qc_reads_device(self._ctx, _ptr(d_words), _ptr(d_quals), _ptr(d_offsets), nreads, _ptr(d_ranges),
                                                     _ptr(d_classes), ctypes.addressof(prm), _ptr(d_report)))

    # -- an assembly scored against the counted table: a record per sequence, a copy number per node, the spectrum (the rule:
    # include/sdt_gpu.h).  Nothing is written to the table; the tally lives from asm_begin to asm_end
    def asm_begin(self, params=None):
        """params: AsmParams or its fields as a dict; zeroes the tally (one byte per table slot) and the totals"""
        prm = params if isinstance(params, AsmParams) else AsmParams(**(params or {}))
        self._check(self.lib.sdt_gpu_asm_begin(self._ctx, ctypes.addressof(prm)))
        self._asm_rows = prm.rows

    def asm_add(self, words, offsets, records: bool = True):
        """a host batch of sequences of any length -> SEQ_SUPPORT_DTYPE[nseqs], or None with records=False (tally only)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros(n, dtype=SEQ_SUPPORT_DTYPE) if records else None
        self._check(self.lib.sdt_gpu_asm_add(self._ctx, _ptr(words), words.size, _ptr(offsets), n, _ptr(out)))
        return out

    def asm_add_device(self, d_words, d_offsets, nseqs: int, d_out=None):
        """device buffers; d_out None or nseqs records of 32 bytes; asynchronous on the context's stream"""
        self._check(self.lib.sdt_gpu_asm_add_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nseqs, _ptr(d_out)))

    def asm_spectrum(self):
        """-> (matrix uint64[rows, ASM_CN_COLS]: occupied slots by min(count, rows - 1) and min(copy number, 7); totals uint64[4]:
        sequences, k-mers, found, solid over all adds since asm_begin)"""
        matrix = np.zeros((getattr(self, "_asm_rows", ASM_MAX_ROWS), ASM_CN_COLS), dtype=np.uint64)
        totals = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_asm_spectrum(self._ctx, _ptr(matrix), _ptr(totals)))
        return matrix, totals

    def asm_end(self):
        self._check(self.lib.sdt_gpu_asm_end(self._ctx))

    # -- reads clustered by connected component of the counted k-mer graph (the rule: include/sdt_gpu.h).  Nothing is written to the
    # table; the labels (4 bytes per table slot) live from cluster_begin to cluster_end
    def cluster_begin(self, params=None):
        """params: ClusterParams or its fields as a dict -> info uint64[8]: live nodes, link ends, clusters, nodes of the largest
        cluster, its id, nodes that are not live, 0, 0"""
        prm = params if isinstance(params, ClusterParams) else ClusterParams(**(params or {}))
        info = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_cluster_begin(self._ctx, ctypes.addressof(prm), _ptr(info)))
        return info

    def cluster_components(self, capacity: int = None):
        """-> (keys uint64[C, key_words]: the smallest k-mer of every cluster, in id order; CLUSTER_COMP_DTYPE[C]: count_sum, nodes);
        capacity: the room to offer (SdtError SDT_EFULL when it is too small: e.needed says how many clusters there are)"""
        n = ctypes.c_uint64()
        if capacity is None:
            rc = self.lib.sdt_gpu_cluster_components(self._ctx, None, None, 0, ctypes.byref(n))
            if rc != SDT_OK and rc != SDT_EFULL:
                self._check(rc)
            capacity = n.value
        nw = self.nw
        keys = np.zeros((max(capacity, 1), nw), dtype=np.uint64)
        comp = np.zeros(max(capacity, 1), dtype=CLUSTER_COMP_DTYPE)
        rc = self.lib.sdt_gpu_cluster_components(self._ctx, _ptr(keys), _ptr(comp), capacity, ctypes.byref(n))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = n.value
            raise e
        return keys[: n.value], comp[: n.value]

    def cluster_lookup(self, keys):
        """keys: uint64[n, key_words] (or [n] for one word), either strand -> uint32[n]: the cluster, CLUSTER_NONE for an absent or
        not live k-mer"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        nw = self.nw
        assert keys.size % nw == 0
        n = keys.size // nw
        out = np.full(n, 0xABABABAB, dtype=np.uint32)
        self._check(self.lib.sdt_gpu_cluster_lookup(self._ctx, _ptr(keys) if n else None, n, _ptr(out) if n else None))
        return out

    def cluster_reads(self, words, offsets, paired: bool = False, pick_lo: int = 0, pick_hi: int = 0xFFFFFFFE):
        """-> (READ_CLUSTER_DTYPE[nreads]; keep uint8[nreads]: pick_lo <= unit <= pick_hi; reads kept)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        rec = np.zeros(n, dtype=READ_CLUSTER_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_cluster_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, int(bool(paired)), pick_lo, pick_hi,
                                                   _ptr(rec), _ptr(keep), ctypes.byref(kept)))
        return rec, keep, kept.value

    def cluster_reads_device(self, d_words, d_offsets, nreads: int, d_rec, d_keep=None, paired: bool = False, pick_lo: int = 0,
                             pick_hi: int = 0xFFFFFFFE, wait: bool = True):
        """device buffers; d_rec holds nreads records of 24 bytes, d_keep (optional) nreads bytes -> reads kept (waits for the kernel),
        or None with wait=False (enqueued on the context's stream)"""
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_cluster_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, int(bool(paired)), pick_lo, pick_hi,
                                                          _ptr(d_rec), _ptr(d_keep), ctypes.byref(kept) if wait else None))
        return kept.value if wait else None

    def cluster_kept_reads(self, total_reads: int, pair_ranges=(), pick_lo: int = 0, pick_hi: int = 0xFFFFFFFE, out: np.ndarray = None):
        """the reads kept in HBM; pair_ranges as for select_kept_reads
        -> (READ_CLUSTER_DTYPE[total_reads] by read ordinal, reads seen, reads kept)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_CLUSTER_DTYPE)
        assert out.dtype == READ_CLUSTER_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        ranges = np.ascontiguousarray(np.asarray(pair_ranges, dtype=np.uint64).reshape(-1))
        assert ranges.size % 2 == 0
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_cluster_kept_reads(self._ctx, _ptr(ranges) if ranges.size else None, ranges.size // 2, pick_lo, pick_hi,
                                                        _ptr(out), total_reads, ctypes.byref(n), ctypes.byref(kept)))
        return out, n.value, kept.value

    def cluster_end(self):
        self._check(self.lib.sdt_gpu_cluster_end(self._ctx))

    # -- the bubbles of the counted k-mer graph (the rule: include/sdt_gpu.h).  Nothing is written to the table; the sorted list lives
    # on the device from bubbles_begin to bubbles_end
    def bubbles_begin(self, params=None):
        """params: BubbleParams or its fields as a dict -> info uint64[8]: live nodes, fork sides, branches walked, branches that
        reached a sink, bubbles, bytes of all paths, longest branch, 0"""
        prm = params if isinstance(params, BubbleParams) else BubbleParams(**(params or {}))
        info = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_bubbles_begin(self._ctx, ctypes.addressof(prm), _ptr(info)))
        return info

    def bubbles_fetch(self, first: int, n: int):
        """-> (keys uint64[n, 2, key_words]: source and sink as oriented words; BUBBLE_DTYPE[n]) of bubbles first .. first + n - 1"""
        keys = np.zeros((n, 2, self.nw), dtype=np.uint64)
        rec = np.zeros(n, dtype=BUBBLE_DTYPE)
        self._check(self.lib.sdt_gpu_bubbles_fetch(self._ctx, first, n, _ptr(keys) if n else None, _ptr(rec) if n else None))
        return keys, rec

    def bubbles_paths(self, first: int, n: int, capacity: int = None):
        """-> (bases uint8[offsets[2 n]]: A 0, C 1, T 2, G 3; offsets uint64[2 n + 1]: branch a of bubble first + i is
        bases[offsets[2 i] : offsets[2 i + 1]], branch b the stretch after it).  capacity: the room to offer (default: what is
        needed, asked for first; SdtError SDT_EFULL when it is too small: e.offsets holds the offsets)"""
        offsets = np.zeros(2 * n + 1, dtype=np.uint64)
        if n == 0:
            return np.zeros(0, dtype=np.uint8), offsets
        if capacity is None:
            self._check(self.lib.sdt_gpu_bubbles_paths(self._ctx, first, n, None, 0, _ptr(offsets)))
            capacity = int(offsets[2 * n])
        bases = np.zeros(max(capacity, 1), dtype=np.uint8)
        rc = self.lib.sdt_gpu_bubbles_paths(self._ctx, first, n, _ptr(bases), capacity, _ptr(offsets))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.offsets = offsets
            raise e
        return bases[: int(offsets[2 * n])], offsets

    def bubbles_end(self):
        self._check(self.lib.sdt_gpu_bubbles_end(self._ctx))

    # -- the unitigs of the counted k-mer graph and their links (the rule: include/sdt_gpu.h).  Nothing is written to the table; the
    # sorted list lives on the device from unitigs_begin to unitigs_end
    def unitigs_begin(self, params=None):
        """params: UnitigParams or its fields as a dict -> info uint64[8]: live nodes, start words, unitigs, circular ones, the sum of
        their nodes (= live nodes), bytes of all sequences, longest unitig in nodes, 0"""
        prm = params if isinstance(params, UnitigParams) else UnitigParams(**(params or {}))
        info = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_unitigs_begin(self._ctx, ctypes.addressof(prm), _ptr(info)))
        return info

    def unitigs_fetch(self, first: int, n: int):
        """-> (keys uint64[n, 2, key_words]: first and last word as the unitig is read; UNITIG_DTYPE[n]) of unitigs first .. first + n - 1"""
        keys = np.zeros((n, 2, self.nw), dtype=np.uint64)
        rec = np.zeros(n, dtype=UNITIG_DTYPE)
        self._check(self.lib.sdt_gpu_unitigs_fetch(self._ctx, first, n, _ptr(keys) if n else None, _ptr(rec) if n else None))
        return keys, rec

    def unitigs_seqs(self, first: int, n: int, capacity: int = None):
        """-> (bases uint8[offsets[n]]: A 0, C 1, T 2, G 3; offsets uint64[n + 1]: unitig first + i is bases[offsets[i] : offsets[i + 1]],
        nodes + K - 1 of them).  capacity: the room to offer (default: what is needed, asked for first; SdtError SDT_EFULL when it is
        too small: e.offsets holds the offsets)"""
        offsets = np.zeros(n + 1, dtype=np.uint64)
        if n == 0:
            return np.zeros(0, dtype=np.uint8), offsets
        if capacity is None:
            self._check(self.lib.sdt_gpu_unitigs_seqs(self._ctx, first, n, None, 0, _ptr(offsets)))
            capacity = int(offsets[n])
        bases = np.zeros(max(capacity, 1), dtype=np.uint8)
        rc = self.lib.sdt_gpu_unitigs_seqs(self._ctx, first, n, _ptr(bases), capacity, _ptr(offsets))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.offsets = offsets
            raise e
        return bases[: int(offsets[n])], offsets

    def unitigs_links(self, first: int, n: int, capacity: int = None):
        """-> (UNITIG_LINK_DTYPE[...]: the links that leave unitigs first .. first + n - 1, by (from, orientation, base); the link ends
        of the range whose target begins no unitig).  capacity: the room to offer (default: what is needed, asked for first; SdtError
        SDT_EFULL when it is too small: e.n_links holds the need)"""
        n_links, n_dangling = _c.c_uint64(0), _c.c_uint64(0)
        if n == 0:
            return np.zeros(0, dtype=UNITIG_LINK_DTYPE), 0
        if capacity is None:
            self._check(self.lib.sdt_gpu_unitigs_links(self._ctx, first, n, None, 0, ctypes.byref(n_links), ctypes.byref(n_dangling)))
            capacity = n_links.value
        links = np.zeros(max(capacity, 1), dtype=UNITIG_LINK_DTYPE)
        rc = self.lib.sdt_gpu_unitigs_links(self._ctx, first, n, _ptr(links), capacity, ctypes.byref(n_links), ctypes.byref(n_dangling))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.n_links = n_links.value
            raise e
        return links[: n_links.value], n_dangling.value

    def unitigs_end(self):
        self._check(self.lib.sdt_gpu_unitigs_end(self._ctx))

    # -- reads threaded through that list (the rule: include/sdt_gpu.h): a label per table slot from unitigs_index to unitigs_end
    def unitigs_index(self):
        """-> info uint64[4]: nodes labelled (= the live nodes), unitigs, bytes held (8 per table slot), 0"""
        info = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_unitigs_index(self._ctx, _ptr(info)))
        return info

    def unitigs_lookup(self, keys):
        """keys: uint64[n, key_words] (or [n] for one word), either strand -> UNITIG_POS_DTYPE[n]: unitig, position and o of the word
        as given; UNITIG_NONE and zeros for an absent or not live k-mer"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        nw = self.nw
        assert keys.size % nw == 0
        n = keys.size // nw
        out = np.full(4 * n, 0xABABABAB, dtype=np.uint32).view(UNITIG_POS_DTYPE)
        self._check(self.lib.sdt_gpu_unitigs_lookup(self._ctx, _ptr(keys) if n else None, n, _ptr(out) if n else None))
        return out

    def unitigs_reads(self, words, offsets, capacity: int = None, segments: bool = True):
        """-> (READ_PATH_DTYPE[nreads]; seg_offsets uint64[nreads + 1]; PATH_SEG_DTYPE[seg_offsets[nreads]]: the segments of read r are
        segs[seg_offsets[r] : seg_offsets[r + 1]]).  segments=False: the records and the offsets only (segs is None).  capacity: the
        room to offer (default: what is needed, asked for first; SdtError SDT_EFULL when it is too small: e.rec, e.seg_offsets and
        e.n_segs are complete)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        rec = np.zeros(n, dtype=READ_PATH_DTYPE)
        seg_offsets = np.zeros(n + 1, dtype=np.uint64)
        total = ctypes.c_uint64()
        if not segments or capacity is None:
            self._check(self.lib.sdt_gpu_unitigs_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, _ptr(rec), _ptr(seg_offsets), None, 0,
                                                       ctypes.byref(total)))
            if not segments:
                return rec, seg_offsets, None
            capacity = total.value
        segs = np.zeros(max(capacity, 1), dtype=PATH_SEG_DTYPE)
        rc = self.lib.sdt_gpu_unitigs_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, _ptr(rec), _ptr(seg_offsets), _ptr(segs), capacity,
                                            ctypes.byref(total))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.rec, e.seg_offsets, e.n_segs = rec, seg_offsets, total.value
            raise e
        return rec, seg_offsets, segs[: total.value]

    def unitigs_reads_device(self, d_words, d_offsets, nreads: int, d_rec, d_seg_offsets, d_segs=None, capacity: int = 0):
        """device buffers; d_rec holds nreads records of 24 bytes, d_seg_offsets nreads + 1 uint64, d_segs (optional) capacity records of
        24 bytes -> the segments of all reads (waits for the total; SdtError SDT_EFULL with e.n_segs when d_segs is too small)"""
        total = ctypes.c_uint64()
        rc = self.lib.sdt_gpu_unitigs_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, _ptr(d_rec), _ptr(d_seg_offsets), _ptr(d_segs), capacity,
                                                   ctypes.byref(total))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.n_segs = total.value
            raise e
        return total.value

    # -- what the reads support of that list (the rule: include/sdt_gpu.h): a tally on the device from unitigs_support_begin to
    # unitigs_support_end / unitigs_end; the add forms ADD
    def unitigs_support_begin(self, params=None):
        """params: SupportParams or its fields as a dict (junction_capacity, mate_capacity: the distinct entries the two sets may hold)"""
        prm = params if isinstance(params, SupportParams) else SupportParams(**(params or {}))
        self._check(self.lib.sdt_gpu_unitigs_support_begin(self._ctx, ctypes.addressof(prm)))

    def unitigs_support_add(self, words, offsets, paired: bool = False):
        """a host batch; paired: reads 2r and 2r + 1 are mates.  SdtError SDT_EFULL when a set has filled up"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_unitigs_support_add(self._ctx, _ptr(words), words.size, _ptr(offsets), len(offsets) - 1, int(paired)))

    def unitigs_support_add_device(self, d_words, d_offsets, nreads: int, paired: bool = False):
        self._check(self.lib.sdt_gpu_unitigs_support_add_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, int(paired)))

    def unitigs_support_unitigs(self, first: int, n: int):
        """-> UNITIG_SUPPORT_DTYPE[n]: the segments and their k-mers in unitigs first .. first + n - 1"""
        out = np.zeros(n, dtype=UNITIG_SUPPORT_DTYPE)
        self._check(self.lib.sdt_gpu_unitigs_support_unitigs(self._ctx, first, n, _ptr(out) if n else None))
        return out

    def unitigs_support_links(self, first: int, n: int, capacity: int = None):
        """-> LINK_SUPPORT_DTYPE[...] parallel to unitigs_links(first, n).  capacity: the room to offer (default: what is needed, asked
        for first; SdtError SDT_EFULL when it is too small: e.n_links holds the need)"""
        n_links = _c.c_uint64(0)
        if n == 0:
            return np.zeros(0, dtype=LINK_SUPPORT_DTYPE)
        if capacity is None:
            self._check(self.lib.sdt_gpu_unitigs_support_links(self._ctx, first, n, None, 0, ctypes.byref(n_links)))
            capacity = n_links.value
        out = np.zeros(max(capacity, 1), dtype=LINK_SUPPORT_DTYPE)
        rc = self.lib.sdt_gpu_unitigs_support_links(self._ctx, first, n, _ptr(out), capacity, ctypes.byref(n_links))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.n_links = n_links.value
            raise e
        return out[: n_links.value]

    def _support_list(self, fn, dtype, capacity):
        n = _c.c_uint64(0)
        if capacity is None:
            self._check(fn(self._ctx, None, 0, ctypes.byref(n)))
            capacity = n.value
        out = np.zeros(max(capacity, 1), dtype=dtype)
        rc = fn(self._ctx, _ptr(out), capacity, ctypes.byref(n))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.n = n.value
            raise e
        return out[: n.value]

    def unitigs_support_junctions(self, capacity: int = None):
        """-> UNITIG_JUNCTION_DTYPE[...], ascending by (via, from, to); SdtError SDT_EFULL when the set filled up or capacity is too small"""
        return self._support_list(self.lib.sdt_gpu_unitigs_support_junctions, UNITIG_JUNCTION_DTYPE, capacity)

    def unitigs_support_mates(self, capacity: int = None):
        """-> MATE_LINK_DTYPE[...], ascending by (from, to)"""
        return self._support_list(self.lib.sdt_gpu_unitigs_support_mates, MATE_LINK_DTYPE, capacity)

    def unitigs_support_totals(self):
        """-> uint64[12], named by SUPPORT_TOTALS"""
        totals = np.zeros(12, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_unitigs_support_totals(self._ctx, _ptr(totals)))
        return totals

    def unitigs_support_end(self):
        self._check(self.lib.sdt_gpu_unitigs_support_end(self._ctx))

    # -- this context's counted table against another's (the rule: include/sdt_gpu.h); nothing is written to either
    def compare(self, other, rows: int = 64, cols: int = 64):
        return compare_tables(self, other, rows, cols)

    def compare_select(self, other, min_a: int = 1, max_a: int = 2**32 - 1, min_b: int = 0, max_b: int = 0, capacity=None):
        return compare_select(self, other, min_a, max_a, min_b, max_b, capacity)

    # -- the mates of an overlapping pair merged into one fragment read by their overlap records; qualities through a compaction (the
    # rule: include/sdt_gpu.h)
    @staticmethod
    def _merge_params(params):
        """params: MergeParams or its fields as a dict"""
        return params if isinstance(params, MergeParams) else MergeParams(**(params or {}))

    def _merge_error(self, rc, n_merged, n_words):
        e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
        e.needed, e.n_merged = n_words.value, n_merged.value
        return e

    def merge_pairs(self, words, offsets, ov, quals=None, params=None, out_words_cap: int = None):
        """reads 2t and 2t + 1 are mates, ov their READ_OVERLAP_DTYPE records, quals (optional) one byte per base under offsets
        -> (READ_MERGE_DTYPE[nreads], words uint32[n_out_words + 4] of the merged reads, offsets uint64[n_merged + 1]);
        SdtError SDT_EFULL when out_words_cap is too small: e.needed = the words without the pad, e.n_merged = the pairs that merge"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ov = np.ascontiguousarray(ov, dtype=READ_OVERLAP_DTYPE)
        n = len(offsets) - 1
        assert len(ov) == n
        if quals is not None:
            quals = np.ascontiguousarray(quals, dtype=np.uint8)
            assert quals.size >= (int(offsets[-1]) if n else 0)
        cap = (((int(offsets[-1]) - int(offsets[0]) + 15) >> 4) if n else 0) + 4 if out_words_cap is None else out_words_cap
        mg = np.zeros(n, dtype=READ_MERGE_DTYPE)
        out_words = np.full(max(cap, 1), 0xABABABAB, dtype=np.uint32)
        out_offsets = np.zeros(n // 2 + 1, dtype=np.uint64)
        prm = self._merge_params(params)
        nm, nw = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.sdt_gpu_merge_pairs(self._ctx, _ptr(words), words.size, _ptr(offsets), n, _ptr(ov), _ptr(quals), ctypes.addressof(prm),
                                          _ptr(mg), _ptr(out_words), cap, _ptr(out_offsets), ctypes.byref(nm), ctypes.byref(nw))
        if rc != SDT_OK:
            raise self._merge_error(rc, nm, nw)
        return mg, out_words[: nw.value + 4], out_offsets[: nm.value + 1]

    def merge_pairs_device(self, d_words, d_offsets, nreads: int, d_ov, d_mg, d_out_words, out_words_cap: int, d_out_offsets, d_quals=None,
                           params=None):
        """device buffers; d_ov and d_mg hold nreads records of 24 bytes (d_mg is what compact_trimmed_device takes), d_quals (optional)
        4-byte aligned, d_out_offsets nreads // 2 + 1 words -> (pairs merged, words without the 4 pad words); SdtError SDT_EFULL: e.needed,
        e.n_merged"""
        prm = self._merge_params(params)
        nm, nw = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.sdt_gpu_merge_pairs_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, _ptr(d_ov), _ptr(d_quals),
                                                 ctypes.addressof(prm), _ptr(d_mg), _ptr(d_out_words), out_words_cap, _ptr(d_out_offsets),
                                                 ctypes.byref(nm), ctypes.byref(nw))
        if rc != SDT_OK:
            raise self._merge_error(rc, nm, nw)
        return nm.value, nw.value

    def merge_kept_pairs(self, total_reads: int, ov, pair_ranges=(), params=None, out: np.ndarray = None, out_words_cap: int = 0,
                         out_reads_cap: int = None):
        """the reads kept in HBM; ov: READ_OVERLAP_DTYPE by read ordinal (what overlap_kept_pairs wrote); pair_ranges as there
        -> (READ_MERGE_DTYPE[total_reads] by read ordinal, words of the merged reads with their 4 pad words, offsets uint64[n_merged + 1],
        reads decided); SdtError SDT_EFULL when a capacity is too small: e.needed, e.n_merged"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_MERGE_DTYPE)
        assert out.dtype == READ_MERGE_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        ov = np.ascontiguousarray(ov, dtype=READ_OVERLAP_DTYPE)
        assert len(ov) >= total_reads
        ranges = np.ascontiguousarray(np.asarray(pair_ranges, dtype=np.uint64).reshape(-1))
        assert ranges.size % 2 == 0
        rcap = total_reads // 2 if out_reads_cap is None else out_reads_cap
        out_words = np.full(max(out_words_cap, 1), 0xABABABAB, dtype=np.uint32)
        out_offsets = np.zeros(rcap + 1, dtype=np.uint64)
        prm = self._merge_params(params)
        n, nm, nw = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.sdt_gpu_merge_kept_pairs(self._ctx, ctypes.addressof(prm), _ptr(ranges) if ranges.size else None, ranges.size // 2, _ptr(ov),
                                               _ptr(out), total_reads, _ptr(out_words), out_words_cap, _ptr(out_offsets), rcap, ctypes.byref(n),
                                               ctypes.byref(nm), ctypes.byref(nw))
        if rc != SDT_OK:
            raise self._merge_error(rc, nm, nw)
        return out, out_words[: nw.value + 4], out_offsets[: nm.value + 1], n.value

    def compact_quals_trimmed(self, quals, offsets, recs, out_cap: int = None):
        """the bytes [start, start + len) of every read, by 24-byte records with start and len where READ_TRIM_DTYPE has them, one read
        after the other -> (uint8[bytes kept, zero-padded to a multiple of 4], bytes kept); what compact_trimmed does to the bases under the same records.  SdtError SDT_EFULL when
        out_cap is less than the bytes kept rounded up to 4: e.needed = the bytes kept"""
        quals = np.ascontiguousarray(quals, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        recs = np.ascontiguousarray(recs)
        assert recs.dtype.itemsize == 24 and len(recs) == len(offsets) - 1
        n = len(offsets) - 1
        cap = (quals.size + 3) & ~3 if out_cap is None else out_cap
        out = np.full(max(cap, 1), 0xAB, dtype=np.uint8)
        nb = ctypes.c_uint64()
        rc = self.lib.sdt_gpu_compact_quals_trimmed(self._ctx, _ptr(quals), quals.size, _ptr(offsets), n, _ptr(recs), _ptr(out), cap,
                                                    ctypes.byref(nb))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = nb.value
            raise e
        return out[: (nb.value + 3) & ~3], nb.value

    def compact_quals_trimmed_device(self, d_quals, d_offsets, nreads: int, d_recs, d_out_quals, out_cap: int) -> int:
        """device buffers; d_out_quals 4-byte aligned, out_cap bytes -> bytes kept (the output is zero-padded to a multiple of 4);
        SdtError SDT_EFULL: e.needed = the bytes kept"""
        nb = ctypes.c_uint64()
        rc = self.lib.sdt_gpu_compact_quals_trimmed_device(self._ctx, _ptr(d_quals), _ptr(d_offsets), nreads, _ptr(d_recs), _ptr(d_out_quals),
                                                           out_cap, ctypes.byref(nb))
        if rc != SDT_OK:
            e = SdtError(rc, self.lib.sdt_gpu_last_error().decode())
            e.needed = nb.value
            raise e
        return nb.value

    # -- reads screened against reference sequences (rRNA, PhiX, ...); a k-mer set of its own, no counted table (the rule: include/sdt_gpu.h)
    @staticmethod
    def _screen_params(params):
        """params: ScreenParams or its fields as a dict"""
        return params if isinstance(params, ScreenParams) else ScreenParams(**(params or {}))

    def screen_load(self, words, offsets, ref_of_seq, n_refs: int, k: int = 31) -> int:
        """sequences packed like reads (with the pad words), ref_of_seq[i] < n_refs -> the distinct k-mers of the set"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        ref_of_seq = np.ascontiguousarray(ref_of_seq, dtype=np.uint32)
        assert len(ref_of_seq) == len(offsets) - 1
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_screen_load(self._ctx, _ptr(words), words.size, _ptr(offsets), len(offsets) - 1, _ptr(ref_of_seq), n_refs, k,
                                                 ctypes.byref(n)))
        return n.value

    def screen_unload(self):
        self._check(self.lib.sdt_gpu_screen_unload(self._ctx))

    def screen_info(self):
        """-> (k, n_refs, distinct k-mers, slots); all 0 without a set"""
        info = (ctypes.c_uint64 * 4)()
        self._check(self.lib.sdt_gpu_screen_info(self._ctx, info))
        return tuple(int(v) for v in info)

    def screen_lookup(self, keys) -> np.ndarray:
        """right-aligned k-mers of either strand -> uint32[n]: the smallest reference that holds each, SCREEN_NO_REF: absent"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        refs = np.zeros(keys.size, dtype=np.uint32)
        self._check(self.lib.sdt_gpu_screen_lookup(self._ctx, _ptr(keys), keys.size, _ptr(refs)))
        return refs

    def screen_reads(self, words, offsets, paired: bool = False, params=None):
        """-> (READ_SCREEN_DTYPE[nreads]: kmers, hits, ref, start, len, verdict; keep uint8[nreads]; reads kept)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        out = np.zeros(n, dtype=READ_SCREEN_DTYPE)
        keep = np.zeros(n, dtype=np.uint8)
        prm = self._screen_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_screen_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), n, int(bool(paired)), ctypes.addressof(prm),
                                                  _ptr(out), _ptr(keep), ctypes.byref(kept)))
        return out, keep, kept.value

    def screen_reads_device(self, d_words, d_offsets, nreads: int, d_out, d_keep=None, paired: bool = False, params=None) -> int:
        """device buffers; d_out holds nreads records of 24 bytes (what compact_trimmed_device takes), d_keep (optional) nreads bytes
        (what compact_reads_device takes) -> reads kept (waits for the kernel)"""
        prm = self._screen_params(params)
        kept = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_screen_reads_device(self._ctx, _ptr(d_words), _ptr(d_offsets), nreads, int(bool(paired)), ctypes.addressof(prm),
                                                         _ptr(d_out), _ptr(d_keep), ctypes.byref(kept)))
        return kept.value

    def screen_kept_reads(self, total_reads: int, pair_ranges=(), params=None, out: np.ndarray = None):
        """the reads kept in HBM; pair_ranges: [first, end) of ordinals that hold interleaved pairs, flat or as rows
        -> (READ_SCREEN_DTYPE[total_reads] by read ordinal, reads decided, reads kept)"""
        if out is None:
            out = np.zeros(total_reads, dtype=READ_SCREEN_DTYPE)
        assert out.dtype == READ_SCREEN_DTYPE and out.flags.c_contiguous and len(out) >= total_reads
        ranges = np.ascontiguousarray(np.asarray(pair_ranges, dtype=np.uint64).reshape(-1))
        assert ranges.size % 2 == 0
        prm = self._screen_params(params)
        n, kept = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_screen_kept_reads(self._ctx, ctypes.addressof(prm), _ptr(ranges) if ranges.size else None, ranges.size // 2,
                                                       _ptr(out), total_reads, ctypes.byref(n), ctypes.byref(kept)))
        return out, n.value, kept.value

    def set_read_ordinal(self, base: int, stride: int = 1):
        self._check(self.lib.sdt_gpu_set_read_ordinal(self._ctx, base, stride))

    # -- pass 2: reads -> edge paths -> arcs (prlRead2edge); see include/sdt_gpu.h for the path word and the patch table
    def _patch_args(self, patch_keys, patch_info):
        if patch_keys is None or len(patch_keys) == 0:
            return None, None, 0
        patch_keys = np.ascontiguousarray(patch_keys, dtype=np.uint64).reshape(-1, self.nw)
        patch_info = np.ascontiguousarray(patch_info, dtype=np.uint64)
        assert len(patch_keys) == len(patch_info)
        return patch_keys, patch_info, len(patch_info)

    def load_paths(self, keys, path_words, patch_keys=None, patch_info=None, num_ed: int = 0, n: int = None):
        """keys None: path_words[i] belongs to node i of set_node_index / layout_apply; path_words None as well: the path words
        build_edges left on the device, for the n nodes of the numbering (default: all of them)"""
        if keys is not None:
            keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.nw)
        if path_words is not None:
            path_words = np.ascontiguousarray(path_words, dtype=np.uint64)
            assert keys is None or len(keys) == len(path_words)
            n = len(path_words)
        elif n is None:
            n = getattr(self, "_nidx", 0)
        pk, pi, npatch = self._patch_args(patch_keys, patch_info)
        self._check(self.lib.sdt_gpu_load_paths(self._ctx, _ptr(keys), _ptr(path_words), n, _ptr(pk), _ptr(pi), npatch, num_ed))

    def map_reads(self):
        """-> (kept reads the pass went over, distinct arcs)"""
        reads, arcs = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_map_reads(self._ctx, ctypes.byref(reads), ctypes.byref(arcs)))
        self._narcs = arcs.value
        return reads.value, arcs.value

    def export_arcs(self, max_arcs: int = None):
        """-> (from, to, mult uint32[n], first uint64[n]) in *.preArc's order; max_arcs: the capacity to offer (default: what the
        last map_reads counted)"""
        if max_arcs is None:
            max_arcs = self._narcs
        m = max(max_arcs, 1)
        fr, to, mult = (np.zeros(m, dtype=np.uint32) for _ in range(3))
        first = np.zeros(m, dtype=np.uint64)
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_export_arcs(self._ctx, _ptr(fr), _ptr(to), _ptr(mult), _ptr(first), max_arcs, ctypes.byref(n)))
        return fr[: n.value], to[: n.value], mult[: n.value], first[: n.value]

    def export_paths(self):
        """-> (keys uint64[n, nw], path_words uint64[n]) of every node, after load_paths"""
        n = ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_export_paths(self._ctx, None, None, 0, ctypes.byref(n)))
        m = max(n.value, 1)
        keys = np.zeros((m, self.nw), dtype=np.uint64)
        words = np.zeros(m, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_export_paths(self._ctx, _ptr(keys), _ptr(words), m, ctypes.byref(n)))
        return keys[: n.value], words[: n.value]

    def import_paths(self, keys, path_words, patch_keys=None, patch_info=None, num_ed: int = 0):
        """the whole graph into a context that holds (its share of) the reads: the table it had makes way"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, self.nw)
        path_words = np.ascontiguousarray(path_words, dtype=np.uint64)
        assert len(keys) == len(path_words)
        pk, pi, npatch = self._patch_args(patch_keys, patch_info)
        self._check(self.lib.sdt_gpu_import_paths(self._ctx, _ptr(keys), _ptr(path_words), len(path_words), _ptr(pk), _ptr(pi), npatch,
                                                  num_ed))

    def keep_reads(self, words: np.ndarray, offsets: np.ndarray):
        """keep a batch resident for map_reads without counting it (ordinals from set_read_ordinal, as for a push)"""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_keep_reads(self._ctx, _ptr(words), words.size, _ptr(offsets), offsets.size - 1))

    def release_table(self):
        self._check(self.lib.sdt_gpu_release_table(self._ctx))

    # -- introspection
    def table_slots(self) -> int:
        return self.lib.sdt_gpu_table_slots(self._ctx)

    def table_info(self) -> dict:
        """layout of the node table as it stands (sdt_gpu_table_info)"""
        a = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.sdt_gpu_table_info(self._ctx, a.ctypes.data))
        return {"layout": "flat", "slots": int(a[1]), "nodes": int(a[2])}

    def stream(self) -> int:
        return self.lib.sdt_gpu_stream(self._ctx) or 0

    def set_stream(self, hip_stream: int):
        self._check(self.lib.sdt_gpu_set_stream(self._ctx, ctypes.c_void_p(hip_stream)))

    def kernel_time(self, reset: bool = True):
        ms, launches, kmers = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self.lib.sdt_gpu_kernel_time(self._ctx, int(reset), ctypes.byref(ms), ctypes.byref(launches),
                                                 ctypes.byref(kmers)))
        return ms.value, launches.value, kmers.value

    def stage_times(self):
        """(ms per stage [direct, sk scatter, sk split, sk count, sk fold], pipeline counters) since the last kernel_time(reset=True)"""
        ms = (ctypes.c_double * 5)()
        cnt = (ctypes.c_uint64 * 20)()
        self._check(self.lib.sdt_gpu_stage_times(self._ctx, ms, cnt))
        names = ("merges", "lds_spills", "pool_direct", "early_flushes", "chunks_l1", "chunks_l2", "batches", "batch_kmers", "cnt_ticks_setup",
                 "cnt_ticks_fill", "cnt_ticks_count", "cnt_ticks_merge", "sc_ticks_stage", "sc_ticks_minima", "sc_ticks_starts",
                 "sc_ticks_emit", "distinct_records", "records", "distinct_record_kmers", "host_cleared_slots")
        return [float(x) for x in ms], dict(zip(names, (int(x) for x in cnt)))


def compare_tables(a: PregraphGPU, b: PregraphGPU, rows: int = 64, cols: int = 64, params=None):
    """two counted tables of the same K on one device -> (matrix uint64[rows, cols]: the distinct canonical k-mers of A u B by
    min(cA, rows - 1) and min(cB, cols - 1); totals uint64[8]: nodes in A, in B, in both, sum cA, sum cB, sum min(cA, cB) over the
    shared nodes, sum cA and sum cB over the shared nodes).  params: a CmpParams instead of rows and cols"""
    prm = params if isinstance(params, CmpParams) else CmpParams(rows, cols)
    # (the arrays are sized before the library has checked the params: what it would refuse gets arrays of one cell)
    ok = 0 < prm.rows * prm.cols <= CMP_MAX_CELLS
    matrix = np.zeros((prm.rows, prm.cols) if ok else (1, 1), dtype=np.uint64)
    totals = np.zeros(8, dtype=np.uint64)
    a._check(a.lib.sdt_gpu_compare_tables(a._ctx, b._ctx, ctypes.addressof(prm), _ptr(matrix), _ptr(totals)))
    return matrix, totals


def compare_select(a: PregraphGPU, b: PregraphGPU, min_a: int = 1, max_a: int = 2**32 - 1, min_b: int = 0, max_b: int = 0, capacity=None):
    """the k-mers of A with min_a <= cA <= max_a and min_b <= cB <= max_b (cB = 0: not in B) -> (keys uint64[m, key words] in the
    layout of export_nodes, count_a uint32[m], count_b uint32[m]) in no particular order.  capacity None: the size is asked for
    first and m is the number of matches; else m = min(matches, capacity).  The number of matches itself: compare_select_count"""
    rg = CmpRange(min_a, max_a, min_b, max_b)
    n = ctypes.c_uint64()
    if capacity is None:
        a._check(a.lib.sdt_gpu_compare_select(a._ctx, b._ctx, ctypes.addressof(rg), None, None, None, 0, ctypes.byref(n)))
        capacity = n.value
    m = int(capacity)
    keys = np.zeros((m, a.nw), dtype=np.uint64)
    ca = np.zeros(m, dtype=np.uint32)
    cb = np.zeros(m, dtype=np.uint32)
    if m:
        a._check(a.lib.sdt_gpu_compare_select(a._ctx, b._ctx, ctypes.addressof(rg), _ptr(keys), _ptr(ca), _ptr(cb), m, ctypes.byref(n)))
    m = min(m, n.value)
    return keys[:m], ca[:m], cb[:m]


def compare_select_count(a: PregraphGPU, b: PregraphGPU, min_a: int = 1, max_a: int = 2**32 - 1, min_b: int = 0, max_b: int = 0) -> int:
    """how many k-mers compare_select would give: capacity = 0 with no arrays"""
    rg = CmpRange(min_a, max_a, min_b, max_b)
    n = ctypes.c_uint64()
    a._check(a.lib.sdt_gpu_compare_select(a._ctx, b._ctx, ctypes.addressof(rg), None, None, None, 0, ctypes.byref(n)))
    return n.value


def new_comm_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it and hands the 128 bytes to every rank)"""
    buf = ctypes.create_string_buffer(128)
    if load_library().sdt_gpu_comm_id(buf) != SDT_OK:
        raise SdtError(SDT_EHIP, load_library().sdt_gpu_last_error().decode())
    return buf.raw


def count_plan(off2, kpre2, first_limit, limit, max_launches=4096):
    """the count stage's work items and launches for chunk lists off2 / kpre2 (csrc/sdt_count_plan.h): (items [n, 4] = c0, c1 | whole,
    first and last final bucket; first_item; launch_kmers)"""
    o = np.ascontiguousarray(off2, dtype=np.uint32)
    kp = np.ascontiguousarray(kpre2, dtype=np.uint64)
    nb = len(o) - 1
    assert len(kp) == nb + 1
    cap = nb + int(o[-1]) // 1024 + 2
    items = np.zeros((cap, 4), dtype=np.uint32)
    first = np.zeros(max_launches + 2, dtype=np.uint32)
    lk = np.zeros(max_launches + 2, dtype=np.uint64)
    ni, nl = ctypes.c_uint32(), ctypes.c_uint32()
    rc = load_library().sdt_sk_plan_count_items(o.ctypes.data, kp.ctypes.data, nb, first_limit, limit, max_launches, items.ctypes.data, cap,
                                                first.ctypes.data, lk.ctypes.data, len(first), ctypes.addressof(ni), ctypes.addressof(nl))
    if rc != 0:
        raise SdtError(rc, load_library().sdt_gpu_last_error().decode())
    return items[: ni.value].copy(), first[: nl.value + 1].copy(), lk[: nl.value].copy()


def shard_cut_ranges(mat: np.ndarray, nranks: int) -> np.ndarray:
    """bucket ranges of equal weight from the all-gathered chunk-list offsets (nranks x 257 uint32); host only"""
    m = np.ascontiguousarray(mat, dtype=np.uint32).reshape(nranks, 257)
    r = np.zeros(nranks + 1, dtype=np.uint32)
    rc = load_library().sdt_shard_cut_ranges(m.ctypes.data, nranks, r.ctypes.data)
    if rc != SDT_OK:
        raise SdtError(rc, load_library().sdt_gpu_last_error().decode())
    return r


def shard_plan(mat: np.ndarray, nranks: int, me: int, ranges: np.ndarray, recv_chunks: int, t: int):
    """sub-round t of the exchange as rank `me` sees it: (subrounds, send_begin, send_count, send_at, recv_count, recv_at)"""
    m = np.ascontiguousarray(mat, dtype=np.uint32).reshape(nranks, 257)
    rg = np.ascontiguousarray(ranges, dtype=np.uint32)
    S = ctypes.c_uint32()
    out = [np.zeros(nranks, dtype=np.uint32) for _ in range(5)]
    rc = load_library().sdt_shard_plan(m.ctypes.data, nranks, me, rg.ctypes.data, recv_chunks, t, ctypes.addressof(S),
                                       *[o.ctypes.data for o in out])
    if rc != SDT_OK:
        raise SdtError(rc, load_library().sdt_gpu_last_error().decode())
    return (S.value, *out)


def kmer_owner(key_words_msw_first, K: int, nranks: int) -> int:
    """rank that owns a canonical k-mer under bucket sharding (host copy of the device function)"""
    a = np.ascontiguousarray(key_words_msw_first, dtype=np.uint64)
    return load_library().sdt_kmer_owner(a.ctypes.data, K, nranks)


def kmer_bucket(key_words_msw_first, K: int) -> int:
    """level-1 minimizer bucket (0..255) of a canonical k-mer (host copy of the device function)"""
    a = np.ascontiguousarray(key_words_msw_first, dtype=np.uint64)
    return load_library().sdt_kmer_bucket(a.ctypes.data, K)


def kmer_final_bucket(key_words_msw_first, K: int) -> int:
    """final minimizer bucket (0 .. 2^18 - 1) of a canonical k-mer: the unit of the locality pipeline's count stage"""
    a = np.ascontiguousarray(key_words_msw_first, dtype=np.uint64)
    return load_library().sdt_kmer_final_bucket(a.ctypes.data, K)


def write_kmerfreq(path: str, hist) -> None:
    """freqStat (prlHashReads.c:994-1023): bins 1..255, one "%lld\\n" per line."""
    with open(path, "w") as fo:
        for i in range(1, 256):
            fo.write(f"{int(hist[i])}\n")


def kmerfreq_text(hist) -> str:
    return "".join(f"{int(hist[i])}\n" for i in range(1, 256))

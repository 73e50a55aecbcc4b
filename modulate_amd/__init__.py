"""modulate_amd -- MI355X (gfx950) implementation of Modulate's cipher hot path.

The product is the C-ABI shared library ``libmodgpu.so`` (include/modgpu.h), built from
``modulate_amd/csrc`` with hipcc, plus the C++ host mirror of the reference surface
(``CEncryptionCycler``, the ``CArk`` buffer path) in ``libmodulate_host.so``.  This Python
package is only a ctypes binding over those libraries for the test-suite and ``bench.py``;
there is no Python implementation of the cipher in it, and importing the bindings fails loudly if
the HIP library has not been built.  (The library's own host loop, for machines without a GPU, lives
in libmodgpu.so itself: modgpu_cycle_scalar_host / modgpu_cycle_auto_host, include/modgpu.h.)
"""
from .capi import (  # noqa: F401
    ModGpuError, lib, lib_path, device_count, cycle_host, cycle_device, hdr_decrypt_host,
    hdr_encrypt_host, cycle_parts_host, cycle_parts_device, cycle_batch_device, cycle_host_split, debug_set_batch, cycle_file, cycle_file_to_host, cycle_host_to_file, DeviceBuffer, time_cycle_device, state_at, jump_table,
    KEY_PS3, KEY_PS4, MAGIC_PS3, MAGIC_PS4, as_int32, EXPORTS, TESTING_EXPORTS, cycle_scalar_host, cycle_auto_host,
    path_stats, gpu_required, last_launch, debug_set_launch, debug_set_pinned_mode, debug_set_staged_mode, kernel_source_hash, feed_kernel_source_hash, prepare, host_tunables, debug_inject_failures, debug_inject_failure_at, debug_injection_armed, debug_hold_slots, debug_forbid_worker_threads, debug_set_pcie_grid, debug_set_gpu_node, debug_set_host_tunable, HOST_TUNABLES, STAGE_FILL, STAGE_LAUNCH, STAGE_SYNC, STAGE_DRAIN, STAGE_AFTER_DRAIN, STAGE_STALL, INJECT_PIECE_LAST, INJECT_PIECE_MIDDLE, PinnedBuffer, host_register, host_unregister,
    DEBUG_EXPORTS, FLAVOURS, testing_flavour, use_testing_flavour, active_flavour, debug_set_queue_ring, debug_set_helpers, queue_stats, testing_hooks, min_gpu_bytes,
    cycle_device_to, cycle_batch_device_to, time_cycle_device_to, to_kernel_source_hash, debug_set_to_form, TO_FORMS,
    rekey_device_to, rekey_batch_device_to, time_rekey_device_to, rekey_kernel_source_hash, debug_set_rekey_form, REKEY_FORMS,
    rekey_move_device, move_workspace_bytes, move_status, debug_set_move_grid,
    rekey_move_table_device, rekey_move_table_workspace_bytes, rekey_move_table_validate, rekey_move_table_status, compaction_table,
    rekey_move_table_kernel_source_hash, debug_set_move_table_grid,
    rekey_relayout_table_device, rekey_relayout_table_validate, relayout_table, splice_moves,
    cycle_table_device, time_cycle_table_device, table, table_workspace_bytes, table_status, table_validate, table_kernel_source_hash,
    debug_set_table_grid, TableEntry, TABLE_DTYPE,
    rekey_table_device, time_rekey_table_device, rekey_table, rekey_table_workspace_bytes, rekey_table_validate,
    rekey_table_kernel_source_hash, debug_set_rekey_table_grid, RekeyTableEntry, REKEY_TABLE_DTYPE,
    verify_device, verify_batch_device, verify_results, time_verify_device, verify_kernel_source_hash, debug_set_verify_form,
    VERIFY_RESULT_DTYPE, VERIFY_NONE,
    digest_device, digest_batch_device, digest_results, digest_adler32, time_digest_device, debug_set_digest_grid, DIGEST_RESULT_DTYPE,
    verify_table_device, verify_table_summary, verify_table_workspace_bytes, time_verify_table_device, verify_table_kernel_source_hash,
    debug_set_verify_table_grid, VERIFY_TABLE_SUMMARY_DTYPE,
    digest_table_device, digest_table_workspace_bytes, time_digest_table_device, debug_set_digest_table_grid,
    cycle_digest_table_device, cycle_digest_table_workspace_bytes, time_cycle_digest_table_device, debug_set_cycle_digest_table_grid,
    DIGEST_OUTPUT, DIGEST_INPUT,
    rekey_digest_table_device, rekey_digest_table_workspace_bytes, time_rekey_digest_table_device, debug_set_rekey_digest_table_grid,
    DIGEST_PLAIN,
    digest_check_device, digest_check_result, digest_check_bits_bytes, time_digest_check_device, DIGEST_CHECK_SUMMARY_DTYPE,
    verify_rekey_table_device, verify_rekey_table_workspace_bytes, time_verify_rekey_table_device, rekey_verify_table_kernel_source_hash,
    debug_set_rekey_verify_table_grid,
    verify_rekey_device, verify_rekey_batch_device, time_verify_rekey_device, rekey_verify_kernel_source_hash,
    keep_kernel_source_hash, keep_policy, debug_set_keep, KEEP_OFF,
    cycle_host_to_device, cycle_device_to_host, cycle_host_to_device_list, cycle_device_to_host_list, cycle_host_to_device_list_digest, cycle_device_to_host_list_digest, cycle_file_to_device, cycle_device_to_file, xfer_kernel_source_hash, debug_set_xfer_form, XFER_FORMS,
    host_loop_isa, cycle_scalar_host_isa, device_numa_node, numa_probe, host_policy, host_policy_engine, host_trace, host_trace_read, host_pool_stats, host_chunking, HOST_TRACE_KINDS,
)

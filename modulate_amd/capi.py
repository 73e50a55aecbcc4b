"""ctypes binding over libmodgpu.so -- every call goes through the C ABI of include/modgpu.h.

Nothing is computed in Python: if the library is missing or a call fails, ModGpuError is raised.

Two flavours of the library exist (modulate_amd/csrc/Makefile): the shipped libmodgpu.so, which is what every
call here uses by default, and libmodgpu_testing.so -- the same sources and device code plus the
modgpu_debug_* hooks of include/modgpu_testing.h.  `with testing_flavour():` routes the calls made inside
the block to the testing flavour (both can be loaded in one process); the debug_* functions refuse to run
outside such a block, because the shipped library has no such hooks.
"""
import contextlib
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

KEY_PS3 = 0xC64EED30  # Modulate/Settings.h:19
KEY_PS4 = 0x90CFC0AB  # Modulate/Settings.h:20
MAGIC_PS3 = 0xC64EED30  # Modulate/Settings.h:16
MAGIC_PS4 = 0x6F303F55  # Modulate/Settings.h:17

# every symbol include/modgpu.h declares: (name, restype, argtypes)
_u64, _i32, _int, _vp = ctypes.c_uint64, ctypes.c_int32, ctypes.c_int, ctypes.c_void_p
EXPORTS = {
    "modgpu_abi_version": (_int, []),
    "modgpu_device_count": (_int, []),
    "modgpu_last_error": (ctypes.c_char_p, []),
    "modgpu_cycle_device": (_int, [_vp, _u64, _i32, _u64, _int, _vp]),
    "modgpu_cycle_host": (_int, [_vp, _u64, _i32, _u64, _int]),
    "modgpu_hdr_decrypt_host": (_int, [_vp, _u64, _int]),
    "modgpu_hdr_encrypt_host": (_int, [_vp, _u64, _int, _int]),
    "modgpu_cycle_parts_host": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_u64), _int, _i32, _int]),
    "modgpu_cycle_parts_device": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_int), _int, _i32]),
    "modgpu_cycle_host_split": (_int, [_vp, _u64, _i32, _u64, _int]),
    "modgpu_cycle_batch_device": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_u64), _int, _i32, _int, _vp]),
    "modgpu_cycle_file": (_int, [ctypes.c_char_p, ctypes.c_char_p, _i32, _u64, _int]),
    "modgpu_cycle_file_to_host": (_int, [ctypes.c_char_p, _u64, _vp, _u64, _i32, _u64, _int]),
    "modgpu_cycle_host_to_file": (_int, [_vp, _u64, ctypes.c_char_p, _i32, _u64, _int]),
    "modgpu_alloc": (_int, [ctypes.POINTER(_vp), _u64, _int]),
    "modgpu_free": (_int, [_vp, _int]),
    "modgpu_h2d": (_int, [_vp, _vp, _u64, _int]),
    "modgpu_d2h": (_int, [_vp, _vp, _u64, _int]),
    "modgpu_sync": (_int, [_int, _vp]),
    "modgpu_prepare": (_int, [_int]),
    "modgpu_state_at": (ctypes.c_uint32, [_i32, _u64]),
    "modgpu_jump_table": (_int, [_int, ctypes.POINTER(ctypes.c_uint32), _int]),
    "modgpu_cycle_scalar_host": (_int, [_vp, _u64, _i32, _u64]),
    "modgpu_cycle_auto_host": (_int, [_vp, _u64, _i32, _u64, _int]),
    "modgpu_host_alloc": (_int, [ctypes.POINTER(_vp), _u64]),
    "modgpu_host_free": (_int, [_vp]),
    "modgpu_host_is_pinned": (_int, [_vp, _u64]),
    "modgpu_host_register": (_int, [_vp, _u64]),
    "modgpu_host_unregister": (_int, [_vp]),
    "modgpu_path_stats": (_int, [_vp, _int]),
    "modgpu_gpu_required": (_int, []),
    "modgpu_min_gpu_bytes": (_u64, []),
    "modgpu_host_policy": (ctypes.c_char_p, []),
    "modgpu_host_policy_engine": (_int, [_u64, _int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "modgpu_host_loop_isa": (ctypes.c_char_p, []),
    "modgpu_host_alloc_near": (_int, [ctypes.POINTER(_vp), _u64, _int]),
    "modgpu_host_alloc_parts": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_u64), _int, _int]),
    "modgpu_device_numa_node": (_int, [_int]),
    "modgpu_cycle_device_to": (_int, [_vp, _vp, _u64, _i32, _u64, _int, _vp]),
    "modgpu_cycle_batch_device_to": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_u64), _int, _i32, _int, _vp]),
    "modgpu_rekey_device_to": (_int, [_vp, _vp, _u64, _i32, _u64, _i32, _u64, _int, _vp]),
    "modgpu_rekey_batch_device_to": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                            ctypes.POINTER(_u64), _int, _i32, _i32, _int, _vp]),
    "modgpu_move_workspace_bytes": (_u64, [_u64]),
    "modgpu_rekey_move_device": (_int, [_vp, _vp, _u64, _i32, _u64, _i32, _u64, _vp, _u64, _int, _vp]),
    "modgpu_move_status": (_int, [_vp, _int, ctypes.POINTER(_u64)]),
    "modgpu_cycle_host_to_device": (_int, [_vp, _vp, _u64, _i32, _u64, _int]),
    "modgpu_cycle_device_to_host": (_int, [_vp, _vp, _u64, _i32, _u64, _int]),
    "modgpu_cycle_host_to_device_list": (_int, [_vp, _u64, _int]),
    "modgpu_cycle_device_to_host_list": (_int, [_vp, _u64, _int]),
    "modgpu_cycle_host_to_device_list_digest": (_int, [_vp, _u64, ctypes.c_uint32, _vp, _int]),
    "modgpu_cycle_device_to_host_list_digest": (_int, [_vp, _u64, ctypes.c_uint32, _vp, _int]),
    "modgpu_cycle_file_to_device": (_int, [ctypes.c_char_p, _u64, _vp, _u64, _i32, _u64, _int]),
    "modgpu_cycle_device_to_file": (_int, [_vp, _u64, ctypes.c_char_p, _i32, _u64, _int]),
    "modgpu_table_workspace_bytes": (_u64, [_u64]),
    "modgpu_cycle_table_device": (_int, [_vp, _u64, _vp, _u64, _int, _vp]),
    "modgpu_table_status": (_int, [_vp, _int, ctypes.POINTER(_u64)]),
    "modgpu_table_validate": (_int, [_vp, _u64]),
    "modgpu_rekey_table_workspace_bytes": (_u64, [_u64]),
    "modgpu_rekey_table_device": (_int, [_vp, _u64, _vp, _u64, _int, _vp]),
    "modgpu_rekey_table_validate": (_int, [_vp, _u64]),
    "modgpu_rekey_move_table_workspace_bytes": (_u64, [_u64, _u64]),
    "modgpu_rekey_move_table_device": (_int, [_vp, _u64, _u64, _vp, _u64, _int, _vp]),
    "modgpu_rekey_move_table_validate": (_int, [_vp, _u64]),
    "modgpu_rekey_move_table_status": (_int, [_vp, _int, ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "modgpu_rekey_relayout_table_device": (_int, [_vp, _u64, _u64, _vp, _u64, _int, _vp]),
    "modgpu_rekey_relayout_table_validate": (_int, [_vp, _u64]),
    "modgpu_verify_device": (_int, [_vp, _vp, _u64, _i32, _u64, _vp, _int, _vp]),
    "modgpu_verify_batch_device": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_u64), _int, _i32,
                                          _vp, _int, _vp]),
    "modgpu_verify_results": (_int, [_vp, _u64, _int, _vp]),
    "modgpu_verify_table_workspace_bytes": (_u64, [_u64]),
    "modgpu_verify_table_device": (_int, [_vp, _u64, _vp, _vp, _u64, _int, _vp]),
    "modgpu_verify_table_summary": (_int, [_vp, _int, _vp]),
    "modgpu_verify_rekey_table_workspace_bytes": (_u64, [_u64]),
    "modgpu_verify_rekey_table_device": (_int, [_vp, _u64, _vp, _vp, _u64, _int, _vp]),
    "modgpu_verify_rekey_device": (_int, [_vp, _vp, _u64, _i32, _u64, _i32, _u64, _vp, _int, _vp]),
    "modgpu_verify_rekey_batch_device": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_u64),
                                                ctypes.POINTER(_u64), _int, _i32, _i32, _vp, _int, _vp]),
    "modgpu_digest_device": (_int, [_vp, _vp, _u64, _i32, _u64, _vp, _int, _vp]),
    "modgpu_digest_batch_device": (_int, [ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_u64), ctypes.POINTER(_u64), _int, _i32,
                                          _vp, _int, _vp]),
    "modgpu_digest_table_workspace_bytes": (_u64, [_u64]),
    "modgpu_digest_table_device": (_int, [_vp, _u64, _vp, _vp, _u64, _int, _vp]),
    "modgpu_cycle_digest_table_workspace_bytes": (_u64, [_u64]),
    "modgpu_cycle_digest_table_device": (_int, [_vp, _u64, _vp, ctypes.c_uint32, _vp, _u64, _int, _vp]),
    "modgpu_rekey_digest_table_workspace_bytes": (_u64, [_u64]),
    "modgpu_rekey_digest_table_device": (_int, [_vp, _u64, _vp, ctypes.c_uint32, _vp, _u64, _int, _vp]),
    "modgpu_digest_results": (_int, [_vp, _u64, _int, _vp, ctypes.POINTER(ctypes.c_uint32)]),
    "modgpu_digest_adler32": (ctypes.c_uint32, [_vp]),
    "modgpu_digest_check_bits_bytes": (_u64, [_u64]),
    "modgpu_digest_check_device": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _int, _vp]),
    "modgpu_digest_check_summary": (_int, [_vp, _int, _vp]),
}


class TableEntry(ctypes.Structure):
    """modgpu_table_entry_t (include/modgpu.h): 40 bytes."""
    _fields_ = [("dst", _vp), ("src", _vp), ("n", _u64), ("stream_off", _u64), ("key", _i32), ("flags", ctypes.c_uint32)]


# the same layout as a numpy structured dtype: a table built with numpy is the bytes the device reads
TABLE_DTYPE = np.dtype([("dst", "<u8"), ("src", "<u8"), ("n", "<u8"), ("stream_off", "<u8"), ("key", "<i4"), ("flags", "<u4")])
assert TABLE_DTYPE.itemsize == ctypes.sizeof(TableEntry) == 40


class RekeyTableEntry(ctypes.Structure):
    """modgpu_rekey_table_entry_t (include/modgpu.h): 56 bytes."""
    _fields_ = [("dst", _vp), ("src", _vp), ("n", _u64), ("off_from", _u64), ("off_to", _u64), ("key_from", _i32), ("key_to", _i32),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


REKEY_TABLE_DTYPE = np.dtype([("dst", "<u8"), ("src", "<u8"), ("n", "<u8"), ("off_from", "<u8"), ("off_to", "<u8"), ("key_from", "<i4"),
                              ("key_to", "<i4"), ("flags", "<u4"), ("reserved", "<u4")])
assert REKEY_TABLE_DTYPE.itemsize == ctypes.sizeof(RekeyTableEntry) == 56


# modgpu_verify_result_t (include/modgpu.h): 32 bytes
VERIFY_RESULT_DTYPE = np.dtype([("mismatches", "<u8"), ("first_mismatch", "<u8"), ("n", "<u8"), ("reserved", "<u8")])
VERIFY_NONE = 0xFFFFFFFFFFFFFFFF  # first_mismatch of a clean entry
# modgpu_digest_result_t (include/modgpu.h): 32 bytes; only the residues mod 65521 of s1 and s2 are specified
DIGEST_OUTPUT, DIGEST_INPUT = 0, 1  # MODGPU_DIGEST_OUTPUT / _INPUT: which side of the XOR a cycle digest table call's records are of
DIGEST_PLAIN = 2  # MODGPU_DIGEST_PLAIN: a rekey digest table call's records are of the plaintext between the two keystreams
DIGEST_RESULT_DTYPE = np.dtype([("s1", "<u8"), ("s2", "<u8"), ("n", "<u8"), ("reserved", "<u8")])
# modgpu_verify_table_summary_t (include/modgpu.h): 32 bytes
VERIFY_TABLE_SUMMARY_DTYPE = np.dtype([("mismatches", "<u8"), ("first_bad_entry", "<u8"), ("entries", "<u8"), ("reserved", "<u8")])
# modgpu_digest_check_summary_t (include/modgpu.h): 32 bytes
DIGEST_CHECK_SUMMARY_DTYPE = np.dtype([("bad_entries", "<u8"), ("first_bad_entry", "<u8"), ("entries", "<u8"), ("refused", "<u8")])


class PathStats(ctypes.Structure):
    """modgpu_path_stats_t (include/modgpu.h)."""
    _fields_ = [(k, _u64) for k in ("gpu_calls", "gpu_bytes", "gpu_launches", "scalar_calls", "scalar_bytes",
                                    "staged_bytes", "direct_bytes", "auto_fallbacks", "auto_small", "auto_policy_host", "midcall_rescues", "midcall_rescued_bytes")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class HostTraceEvent(ctypes.Structure):
    """modgpu_host_trace_event_t (include/modgpu_testing.h)."""
    _fields_ = [("t_ns", _u64), ("kind", _int), ("pipe", _int), ("chunk", _u64), ("bytes", _u64), ("tid", _int), ("reserved", _int)]


HOST_TRACE_KINDS = ("call_begin", "slots", "posted", "pipe_start", "fill_begin", "fill_end", "launched", "sync_begin", "sync_end",
                    "drain_end", "pipe_end", "call_end", "failed", "rescued", "ready")


class LaunchInfo(ctypes.Structure):
    """modgpu_launch_info_t (include/modgpu_testing.h)."""
    _fields_ = [("kernel", ctypes.c_char_p), ("variant", _int), ("grid", ctypes.c_uint32), ("block", ctypes.c_uint32),
                ("chunk_bytes", ctypes.c_uint32), ("bytes", _u64), ("main_groups", ctypes.c_uint32), ("source_hash", ctypes.c_char_p)]


# include/modgpu_testing.h, reporting group: in both flavours (measurement, not the drop-in boundary)
TESTING_EXPORTS = {
    "modgpu_time_cycle_device": (_int, [_vp, _u64, _i32, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_last_launch": (_int, [ctypes.POINTER(LaunchInfo)]),
    "modgpu_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_feed_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_host_tunables": (None, [ctypes.POINTER(_u64)]),
    "modgpu_host_chunking": (None, [ctypes.POINTER(_u64)]),
    "modgpu_host_loop_info": (None, [ctypes.POINTER(_u64)]),
    "modgpu_host_trace": (None, [_int]),
    "modgpu_host_trace_read": (_int, [ctypes.POINTER(HostTraceEvent), _int]),
    "modgpu_host_pool_stats": (None, [ctypes.POINTER(_u64)]),
    "modgpu_cycle_scalar_host_isa": (_int, [_vp, _u64, _i32, _u64, ctypes.c_char_p]),
    "modgpu_queue_stats": (None, [ctypes.POINTER(_u64)]),
    "modgpu_host_alloc_on_node": (_int, [ctypes.POINTER(_vp), _u64, _int]),
    "modgpu_testing_hooks": (_int, []),
    "modgpu_numa_probe": (_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(_int), ctypes.POINTER(_int), _int]),
    "modgpu_time_cycle_device_to": (_int, [_vp, _vp, _u64, _i32, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_to_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_xfer_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_time_rekey_device_to": (_int, [_vp, _vp, _u64, _i32, _u64, _i32, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_rekey_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_time_cycle_table_device": (_int, [_vp, _u64, _vp, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_table_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_time_rekey_table_device": (_int, [_vp, _u64, _vp, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_rekey_table_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_time_verify_device": (_int, [_vp, _vp, _u64, _i32, _u64, _vp, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_verify_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_time_verify_table_device": (_int, [_vp, _u64, _vp, _vp, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_verify_table_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_time_digest_table_device": (_int, [_vp, _u64, _vp, _vp, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_time_cycle_digest_table_device": (_int, [_vp, _u64, _vp, ctypes.c_uint32, _vp, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_time_rekey_digest_table_device": (_int, [_vp, _u64, _vp, ctypes.c_uint32, _vp, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_time_verify_rekey_device": (_int, [_vp, _vp, _u64, _i32, _u64, _i32, _u64, _vp, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_rekey_verify_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_keep_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_time_verify_rekey_table_device": (_int, [_vp, _u64, _vp, _vp, _u64, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_rekey_verify_table_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_rekey_move_table_kernel_source_hash": (ctypes.c_char_p, []),
    "modgpu_keep_policy": (_int, [_u64, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]),
    "modgpu_time_digest_device": (_int, [_vp, _vp, _u64, _i32, _u64, _vp, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
    "modgpu_time_digest_check_device": (_int, [_vp, _vp, _u64, _vp, _vp, _vp, _int, _vp, _int, ctypes.POINTER(ctypes.c_float)]),
}
# include/modgpu_testing.h, modgpu_debug_* group: ONLY in libmodgpu_testing.so
DEBUG_EXPORTS = {
    "modgpu_debug_set_launch": (None, [_int, ctypes.c_uint32]),
    "modgpu_debug_set_pinned_mode": (None, [_int]),
    "modgpu_debug_set_staged_mode": (None, [_int]),
    "modgpu_debug_set_queue_ring": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_helpers": (None, [_int]),
    "modgpu_debug_set_batch": (None, [_int]),
    "modgpu_debug_set_pcie_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_gpu_node": (None, [_int]),
    "modgpu_debug_set_host_tunable": (None, [_int, _u64]),
    "modgpu_debug_inject_failures": (None, [_int]),
    "modgpu_debug_inject_failure_at": (None, [ctypes.c_int64, _int]),
    "modgpu_debug_injection_armed": (_int, []),
    "modgpu_debug_hold_slots": (_int, [_int, _int]),
    "modgpu_debug_forbid_worker_threads": (None, [_int]),
    "modgpu_debug_set_to_form": (None, [_int]),
    "modgpu_debug_set_xfer_form": (None, [_int]),
    "modgpu_debug_set_rekey_form": (None, [_int]),
    "modgpu_debug_set_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_rekey_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_move_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_move_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_verify_form": (None, [_int]),
    "modgpu_debug_set_verify_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_rekey_verify_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_digest_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_cycle_digest_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_rekey_digest_table_grid": (None, [ctypes.c_uint32]),
    "modgpu_debug_set_keep": (None, [_u64, ctypes.c_uint32, ctypes.c_uint32]),
    "modgpu_debug_set_digest_grid": (None, [_int]),
}


class ModGpuError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"modgpu error {code}: {text}")
        self.code = code


FLAVOURS = {"shipped": "libmodgpu.so", "testing": "libmodgpu_testing.so"}


def lib_path(flavour="shipped"):
    # MODGPU_LIB: another build of the same sources stands in for both flavours (the sanitizer builds of
    # `make sanitize-lib`, which carry the hooks; tests/test_sanitizers.py)
    return os.environ.get("MODGPU_LIB") or os.path.join(_HERE, FLAVOURS[flavour])


_libs = {}
_active = "shipped"


def _load(flavour):
    if flavour not in _libs:
        path = lib_path(flavour)
        if not os.path.exists(path):
            raise ModGpuError(-1, f"{path} not built: run `make -C modulate_amd/csrc` (the Python package has no implementation of its own)")
        L = ctypes.CDLL(path)
        table = list(EXPORTS.items()) + list(TESTING_EXPORTS.items()) + (list(DEBUG_EXPORTS.items()) if flavour == "testing" else [])
        for name, (res, args) in table:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _libs[flavour] = L
    return _libs[flavour]


def lib():
    """The library calls go to: the shipped libmodgpu.so, or libmodgpu_testing.so inside `testing_flavour()`.
    Raises if it was not built (python __graft_entry__.py build)."""
    return _load(_active)


def active_flavour():
    return _active


@contextlib.contextmanager
def testing_flavour():
    """Calls made inside the block go to libmodgpu_testing.so (the flavour that has the modgpu_debug_* hooks).
    Buffers created inside keep using it after the block (they remember their library)."""
    global _active
    prev, _active = _active, "testing"
    try:
        yield _load("testing")
    finally:
        _active = prev


def use_testing_flavour():
    """For tools/: switch this process to libmodgpu_testing.so for good."""
    global _active
    _active = "testing"
    return _load("testing")


def _debug_lib():
    if _active != "testing":
        raise ModGpuError(-1, "modgpu_debug_* hooks exist only in libmodgpu_testing.so: call inside `with testing_flavour():`")
    return _load("testing")


def as_int32(key):
    key &= 0xFFFFFFFF
    return key - (1 << 32) if key & 0x80000000 else key


def _check(rc):
    if rc != 0:
        raise ModGpuError(rc, lib().modgpu_last_error().decode())


def _ptr_array(xs):
    """the void* array of a batch call: the device addresses of `xs` (addresses or DeviceBuffers; a None entry is NULL); None stays None"""
    return (_vp * len(xs))(*[_dev_addr(x) if x is not None else 0 for x in xs]) if xs is not None else None


def _u64_array(xs):
    """the uint64_t array of a batch call (sizes, stream offsets); None stays None"""
    return (_u64 * len(xs))(*xs) if xs is not None else None


def _own_result_call(call, first, src, n, scalars, result, device, stream, fetch, needed="both sides are", first_optional=False):
    """The single-entry calls that write one 32-byte record: library function `call` gets (first, src, n, *scalars, record, device,
    stream).  `first` (the comparand, or the destination, which may be None if `first_optional`) and `src` are addresses or
    DeviceBuffers, and n defaults to the smaller DeviceBuffer's size.  With result=None a record is made, the stream synchronised and
    fetch(record, 1, device) returned (the record is freed whatever happened); otherwise the call is asynchronous and returns None."""
    if n is None:
        if not isinstance(src, DeviceBuffer) or not (isinstance(first, DeviceBuffer) or (first_optional and first is None)):
            raise TypeError(f"n is needed unless {needed} DeviceBuffer")
        n = src.nbytes if first is None else min(first.nbytes, src.nbytes)
    own = DeviceBuffer(32, device) if result is None else None
    try:
        _check(getattr(lib(), call)(_vp(_dev_addr(first) if first is not None else 0), _vp(_dev_addr(src)), n, *scalars,
                                    _vp(_dev_addr(own if own is not None else result)), device, _vp(stream or 0)))
        if own is None:
            return None
        _check(lib().modgpu_sync(device, _vp(stream or 0)))
        return fetch(own, 1, device)
    finally:
        if own is not None:
            own.free()


def _host_ptr(a):
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"] and a.flags["WRITEABLE"]):
        raise TypeError("need a writable C-contiguous uint8 ndarray")
    return ctypes.c_void_p(a.ctypes.data)


def device_count():
    return lib().modgpu_device_count()


def cycle_host(buf, key, stream_off=0, device=-1):
    """In-place CEncryptionCycler::Cycle over a host ndarray, computed on the GPU."""
    _check(lib().modgpu_cycle_host(_host_ptr(buf), buf.size, as_int32(key), stream_off, device))
    return buf


def cycle_scalar_host(buf, key, stream_off=0):
    """The library's own host loop (never the GPU)."""
    _check(lib().modgpu_cycle_scalar_host(_host_ptr(buf), buf.size, as_int32(key), stream_off))
    return buf


def cycle_auto_host(buf, key, stream_off=0, device=-1):
    """What CEncryptionCycler::Cycle binds to: the GPU, the host loop only when no GPU is usable."""
    _check(lib().modgpu_cycle_auto_host(_host_ptr(buf), buf.size, as_int32(key), stream_off, device))
    return buf


def path_stats(reset=False):
    st = PathStats()
    _check(lib().modgpu_path_stats(ctypes.byref(st), 1 if reset else 0))
    return st.as_dict()


def gpu_required():
    return bool(lib().modgpu_gpu_required())


def last_launch():
    info = LaunchInfo()
    _check(lib().modgpu_last_launch(ctypes.byref(info)))
    return {"kernel": info.kernel.decode(), "variant": info.variant, "grid": info.grid, "block": info.block,
            "chunk_bytes": info.chunk_bytes, "bytes": info.bytes, "main_groups": info.main_groups,
            "source_hash": info.source_hash.decode() if info.source_hash else None}


SHAPES = {None: -1, "auto": -1, "small": 0, "large": 1, "queue": 2}


def debug_set_launch(shape=None, grid_cap=0):
    """Test hook: force the launch shape ("small" / "large" = streaming, static chunk map / "queue" = streaming,
    work queue / None = by size) and cap the grid."""
    _debug_lib().modgpu_debug_set_launch(SHAPES[shape], grid_cap or 0)


def debug_set_pinned_mode(mode=0):
    """Test hook: 0 default, 1 DMA pipeline, 2 kernel over PCIe, for pinned caller buffers."""
    _debug_lib().modgpu_debug_set_pinned_mode(mode)


def debug_set_staged_mode(mode=0):
    """Test hook: 0 default, 1 DMA, 2 kernel over PCIe on the pinned slot, for staged (pageable / file) chunks."""
    _debug_lib().modgpu_debug_set_staged_mode(mode)


HOST_TUNABLES = {"zerocopy_bytes": 0, "ring": 1, "split": 2, "chunk_min_bytes": 3, "ramp_bytes": 4, "lanes": 5, "ntcopy": 6, "file_sched": 7,
                 "feed": 8, "feed_chunk_bytes": 9, "feed_patience_ms": 10, "file_feed": 11,
                 "xfer_list_most_bytes": 12}


def debug_set_host_tunable(name, value):
    """Testing flavour: one of HOST_TUNABLES at run time (not while a host-buffer call is in flight)."""
    _debug_lib().modgpu_debug_set_host_tunable(HOST_TUNABLES[name], int(value))


def debug_set_gpu_node(node=-2):
    """Testing flavour: the NUMA node the library believes its GPUs hang off (-2 = ask sysfs)."""
    _debug_lib().modgpu_debug_set_gpu_node(node)


def debug_set_pcie_grid(cap=0):
    """Measurement hook: workgroups of a launch across PCIe (0 = the product's rule)."""
    _debug_lib().modgpu_debug_set_pcie_grid(cap)


def debug_inject_failures(count):
    """Test hook: the next `count` host-buffer / file calls fail with MODGPU_ERR_HIP before touching anything."""
    _debug_lib().modgpu_debug_inject_failures(count)


STAGE_FILL, STAGE_LAUNCH, STAGE_SYNC, STAGE_DRAIN, STAGE_AFTER_DRAIN, STAGE_STALL = range(6)
INJECT_PIECE_LAST, INJECT_PIECE_MIDDLE = -1, -2


def debug_inject_failure_at(piece, stage):
    """Test hook: the HIP call of `stage` (STAGE_*) for piece `piece` of the next host-buffer / file call fails, once.  stage < 0 disarms."""
    _debug_lib().modgpu_debug_inject_failure_at(piece, stage)


def debug_forbid_worker_threads(forbid=True):
    """Testing flavour: staging sets start no worker thread from now on (as if thread creation failed)."""
    _debug_lib().modgpu_debug_forbid_worker_threads(1 if forbid else 0)


def debug_hold_slots(device, count):
    """Testing flavour: hold `count` pipeline slots of a device's staging set (0 releases); returns how many are held."""
    return _debug_lib().modgpu_debug_hold_slots(device, count)


def debug_injection_armed():
    return bool(_debug_lib().modgpu_debug_injection_armed())


def debug_set_helpers(mode=0):
    """Test hook: helper workgroups of the work-queue shape: 0 by the clock they measure, 1 always join, 2 none."""
    _debug_lib().modgpu_debug_set_helpers(mode)


def debug_set_queue_ring(lines=0):
    """Test hook: eager work-queue launches draw ticket pairs from the first `lines` ring lines only (0 = all 4096)."""
    _debug_lib().modgpu_debug_set_queue_ring(lines)


def debug_set_batch(mode=0):
    """Test hook: 0 several parts share a launch beyond 256 MiB in all or when small on average (shipped), 1 always, 2 never."""
    _debug_lib().modgpu_debug_set_batch(mode)


def queue_stats():
    """Work-queue bookkeeping since load (include/modgpu_testing.h: modgpu_queue_stats)."""
    out = (_u64 * 6)()
    lib().modgpu_queue_stats(out)
    return {"eager": int(out[0]), "busy_fallbacks": int(out[1]), "graph": int(out[2]), "graph_pool_empty": int(out[3]),
            "batch_launches": int(out[4]), "batch_parts": int(out[5])}


def testing_hooks():
    return bool(lib().modgpu_testing_hooks())


def min_gpu_bytes():
    return int(lib().modgpu_min_gpu_bytes())


def host_policy():
    """MODGPU_HOST_POLICY as latched: "offload" or "fastest"."""
    return lib().modgpu_host_policy().decode()


def host_policy_engine(n, pinned=False):
    """What `fastest` would decide for one call over n bytes: ("host" | "kernel", host_us, kernel_us)."""
    h, k = ctypes.c_double(0), ctypes.c_double(0)
    r = lib().modgpu_host_policy_engine(n, 1 if pinned else 0, ctypes.byref(h), ctypes.byref(k))
    return ("host" if r else "kernel"), h.value, k.value


def host_loop_isa():
    return lib().modgpu_host_loop_isa().decode()


def cycle_scalar_host_isa(buf, key, isa, stream_off=0):
    """The library's host loop with one named body ("generic" / "avx2" / "avx512")."""
    _check(lib().modgpu_cycle_scalar_host_isa(_host_ptr(buf), buf.size, as_int32(key), stream_off, isa.encode()))
    return buf


def device_numa_node(device):
    return lib().modgpu_device_numa_node(device)


def numa_probe(sysfs_root, bdf, max_cpus=4096):
    """(node, cpus) as the library reads them from a sysfs tree (tests hand it a fake one)."""
    node = _int(-1)
    cpus = (_int * max_cpus)()
    n = lib().modgpu_numa_probe(os.fsencode(sysfs_root), bdf.encode(), ctypes.byref(node), cpus, max_cpus)
    return node.value, list(cpus[:max(n, 0)])


def host_tunables():
    """The host-path tunables as latched (and clamped) at library load."""
    out = (_u64 * 4)()
    lib().modgpu_host_tunables(out)
    return {"pipes": int(out[0]), "chunk_bytes": int(out[1]), "zerocopy_max_bytes": int(out[2]), "ring": int(out[3])}


def host_chunking():
    out = (_u64 * 4)()
    lib().modgpu_host_chunking(out)
    return {"split": int(out[0]), "chunk_min_bytes": int(out[1]), "ramp_bytes": int(out[2]), "lanes": int(out[3])}


def host_trace(enable=True):
    """Start (and clear) / stop the host-side timeline of the host-buffer and file routes."""
    lib().modgpu_host_trace(1 if enable else 0)


def host_trace_read():
    """The recorded events as dicts, in recording order: t_ns, kind (HOST_TRACE_KINDS), pipe (-1: the call), chunk, bytes."""
    n = lib().modgpu_host_trace_read(None, 0)
    buf = (HostTraceEvent * max(n, 1))()
    n = min(lib().modgpu_host_trace_read(buf, n), n)
    return [{"t_ns": int(e.t_ns), "kind": HOST_TRACE_KINDS[e.kind], "pipe": e.pipe, "chunk": int(e.chunk), "bytes": int(e.bytes), "tid": e.tid} for e in buf[:n]]


def host_pool_stats():
    out = (_u64 * 6)()
    lib().modgpu_host_pool_stats(out)
    return {"workers_started": int(out[0]), "pipelines_run_by_workers": int(out[1]), "slot_waits": int(out[2]),
            "calls_overlapped": int(out[3]), "slots_per_device": int(out[4]), "calls_on_another_nodes_set": int(out[5])}


def prepare(device=-1):
    """modgpu_prepare: device preparation + the empty wake-up launch, for callers that bring their own device memory."""
    _check(lib().modgpu_prepare(device))


def kernel_source_hash():
    return lib().modgpu_kernel_source_hash().decode()


def rekey_kernel_source_hash():
    """identity of the rekey kernel's TU (cycle_rekey_kernel.hip and what it includes)"""
    return lib().modgpu_rekey_kernel_source_hash().decode()


def to_kernel_source_hash():
    """identity of the out-of-place kernel's TU (cycle_to_kernel.hip and what it includes)"""
    return lib().modgpu_to_kernel_source_hash().decode()


def xfer_kernel_source_hash():
    """identity of the transfer kernels' TU (cycle_xfer_kernel.hip and what it includes)"""
    return lib().modgpu_xfer_kernel_source_hash().decode()


def feed_kernel_source_hash():
    """identity of the host-fed kernel's TU (cycle_feed_kernel.hip and what it includes)"""
    return lib().modgpu_feed_kernel_source_hash().decode()


class PinnedBuffer:
    """Host memory from modgpu_host_alloc, viewed as a numpy uint8 array (`.array`)."""

    def __init__(self, nbytes, near_device=None, parts=None, n_devices=0):
        """near_device: place the pages next to that GPU (modgpu_host_alloc_near); parts: list of part sizes laid end
        to end, part i next to GPU i mod n_devices (modgpu_host_alloc_parts; nbytes must be their sum)."""
        p = _vp()
        self._lib = lib()
        if parts is not None:
            assert sum(parts) == nbytes
            sizes = (_u64 * len(parts))(*parts)
            _check(self._lib.modgpu_host_alloc_parts(ctypes.byref(p), sizes, len(parts), n_devices))
        elif near_device is not None:
            _check(self._lib.modgpu_host_alloc_near(ctypes.byref(p), nbytes, near_device))
        else:
            _check(self._lib.modgpu_host_alloc(ctypes.byref(p), nbytes))
        self.ptr, self.nbytes = p.value, nbytes
        self.array = np.ctypeslib.as_array(ctypes.cast(self.ptr, ctypes.POINTER(ctypes.c_uint8)), shape=(max(nbytes, 1),))[:nbytes]

    @property
    def pinned(self):
        return bool(self._lib.modgpu_host_is_pinned(_vp(self.ptr), self.nbytes))

    def free(self):
        if self.ptr:
            self.array = None
            _check(self._lib.modgpu_host_free(_vp(self.ptr)))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def host_register(buf):
    """Page-lock a caller-owned ndarray in place (modgpu_host_register); pair with host_unregister(buf)."""
    _check(lib().modgpu_host_register(_host_ptr(buf), buf.size))


def host_unregister(buf):
    _check(lib().modgpu_host_unregister(_host_ptr(buf)))


def hdr_decrypt_host(hdr, device=-1):
    _check(lib().modgpu_hdr_decrypt_host(_host_ptr(hdr), hdr.size, device))
    return hdr


def hdr_encrypt_host(hdr, ps4=True, device=-1):
    _check(lib().modgpu_hdr_encrypt_host(_host_ptr(hdr), hdr.size, 1 if ps4 else 0, device))
    return hdr


def cycle_parts_host(parts, key, n_devices=0):
    n = len(parts)
    ptrs = (_vp * n)(*[_host_ptr(p).value for p in parts])
    sizes = (_u64 * n)(*[p.size for p in parts])
    _check(lib().modgpu_cycle_parts_host(ptrs, sizes, n, as_int32(key), n_devices))
    return parts


def cycle_parts_device(buffers, key):
    """DeviceBuffers, each on its own device: every one cycled as its own stream from offset 0, all GPUs at once."""
    n = len(buffers)
    ptrs = (_vp * n)(*[b.ptr for b in buffers])
    sizes = (_u64 * n)(*[b.nbytes for b in buffers])
    devs = (_int * n)(*[b.device for b in buffers])
    _check(lib().modgpu_cycle_parts_device(ptrs, sizes, devs, n, as_int32(key)))


def cycle_host_split(buf, key, stream_off=0, n_devices=0):
    """One host buffer over several GPUs: contiguous spans, span d on GPU d with its own stream offset (no exchange step)."""
    _check(lib().modgpu_cycle_host_split(_host_ptr(buf), buf.size, as_int32(key), stream_off, n_devices))
    return buf


def cycle_batch_device(ptrs, sizes, key, stream_offs=None, device=-1, stream=None):
    """Raw device addresses of ONE device, each its own Cycle call (from stream_offs[i] or 0); asynchronous on `stream`.
    Runs of up to 16 parts share one kernel launch when together they are beyond 256 MiB or small on average."""
    _check(lib().modgpu_cycle_batch_device(_ptr_array(ptrs), _u64_array(sizes), _u64_array(stream_offs), len(ptrs), as_int32(key), device,
                                           _vp(stream or 0)))


def cycle_file(src_path, dst_path, key, stream_off=0, device=-1):
    """Stream a whole part file through the GPU (dst may equal src: in place)."""
    _check(lib().modgpu_cycle_file(os.fsencode(src_path), os.fsencode(dst_path), as_int32(key), stream_off, device))


def cycle_file_to_host(path, n, key, file_off=0, stream_off=0, device=-1, out=None):
    """n bytes of a part file through the GPU into host memory (`out`: a caller array, e.g. a view of a PinnedBuffer)."""
    if out is None:
        out = np.empty(n, dtype=np.uint8)
    assert out.dtype == np.uint8 and out.size == n and out.flags["C_CONTIGUOUS"]
    _check(lib().modgpu_cycle_file_to_host(os.fsencode(path), file_off, _vp(out.ctypes.data), n, as_int32(key),
                                           stream_off, device))
    return out


def cycle_host_to_file(buf, path, key, stream_off=0, device=-1):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    _check(lib().modgpu_cycle_host_to_file(_vp(buf.ctypes.data), buf.size, os.fsencode(path), as_int32(key),
                                           stream_off, device))


def cycle_device(dev_ptr, n, key, stream_off=0, device=-1, stream=None):
    """Asynchronous in-place cycle of n device-resident bytes at raw address dev_ptr."""
    _check(lib().modgpu_cycle_device(_vp(dev_ptr), n, as_int32(key), stream_off, device, _vp(stream or 0)))


def time_cycle_device(dev_ptr, n, key, stream_off=0, device=-1, stream=None, iters=2):
    """Mean ms per launch over `iters` launches, HIP events on the launch stream."""
    return _time_call("modgpu_time_cycle_device", (_vp(dev_ptr), n, as_int32(key), stream_off), device, stream, iters)


def cycle_device_to(dst_ptr, src_ptr, n, key, stream_off=0, device=-1, stream=None):
    """Asynchronous OUT-OF-PLACE cycle: dst[j] = src[j] ^ ks[stream_off + j] for n bytes at raw device addresses; src is not
    modified (dst == src is the in-place call; a partial overlap is refused)."""
    _check(lib().modgpu_cycle_device_to(_vp(dst_ptr), _vp(src_ptr), n, as_int32(key), stream_off, device, _vp(stream or 0)))


def cycle_batch_device_to(dst_ptrs, src_ptrs, sizes, key, stream_offs=None, device=-1, stream=None):
    """Several out-of-place entries of ONE device (entry i from stream_offs[i] or 0); sources may overlap each other, a
    destination may meet no other entry's range.  Up to 16 non-empty entries share a launch."""
    n = len(dst_ptrs)
    assert len(src_ptrs) == n and len(sizes) == n
    _check(lib().modgpu_cycle_batch_device_to(_ptr_array(dst_ptrs), _ptr_array(src_ptrs), _u64_array(sizes), _u64_array(stream_offs), n,
                                              as_int32(key), device, _vp(stream or 0)))


def time_cycle_device_to(dst_ptr, src_ptr, n, key, stream_off=0, device=-1, stream=None, iters=2):
    """Mean ms per out-of-place launch over `iters` launches, HIP events on the launch stream."""
    return _time_call("modgpu_time_cycle_device_to", (_vp(dst_ptr), _vp(src_ptr), n, as_int32(key), stream_off), device, stream, iters)


def rekey_device_to(dst, src, key_from, key_to, off_from=0, off_to=0, device=-1, stream=None, *, n=None):
    """Asynchronous REKEY of n bytes at raw device addresses: dst[j] = src[j] ^ ks(key_from)[off_from + j] ^ ks(key_to)[off_to + j], in
    one pass; src is not modified (dst == src rekeys in place; a partial overlap is refused).  `dst` / `src` are addresses or
    DeviceBuffer; n defaults to the smaller buffer's size when both are DeviceBuffer."""
    if n is None:
        if not (isinstance(dst, DeviceBuffer) and isinstance(src, DeviceBuffer)):
            raise TypeError("n is needed unless both sides are DeviceBuffer")
        n = min(dst.nbytes, src.nbytes)
    _check(lib().modgpu_rekey_device_to(_vp(_dev_addr(dst)), _vp(_dev_addr(src)), n, as_int32(key_from), off_from, as_int32(key_to), off_to,
                                        device, _vp(stream or 0)))


def rekey_batch_device_to(dst_ptrs, src_ptrs, sizes, key_from, key_to, offs_from=None, offs_to=None, device=-1, stream=None):
    """Several rekey entries of ONE device (entry i from offs_from[i] / offs_to[i], or 0); sources may overlap each other, a destination
    may meet no other entry's range.  Up to 16 non-empty entries share a launch."""
    n = len(dst_ptrs)
    assert len(src_ptrs) == n and len(sizes) == n
    _check(lib().modgpu_rekey_batch_device_to(_ptr_array(dst_ptrs), _ptr_array(src_ptrs), _u64_array(sizes), _u64_array(offs_from),
                                              _u64_array(offs_to), n, as_int32(key_from), as_int32(key_to), device, _vp(stream or 0)))


def time_rekey_device_to(dst, src, n, key_from, key_to, off_from=0, off_to=0, device=-1, stream=None, iters=2):
    """Mean ms per rekey launch over `iters` launches, HIP events on the launch stream."""
    return _time_call("modgpu_time_rekey_device_to", (_vp(_dev_addr(dst)), _vp(_dev_addr(src)), n, as_int32(key_from), off_from, as_int32(key_to),
                                                      off_to), device, stream, iters)


def move_workspace_bytes(n):
    """bytes of device workspace rekey_move_device needs for n bytes (0 for n == 0, or an entry of 2^24 chunks or more)"""
    return lib().modgpu_move_workspace_bytes(n)


def rekey_move_device(dst, src, n, key_from, key_to, off_from=0, off_to=0, workspace=None, device=-1, stream=None):
    """Asynchronous REKEY of n bytes at raw device addresses with memmove rules: dst[j] = SRC0[j] ^ ks(key_from)[off_from + j] ^
    ks(key_to)[off_to + j] for ANY overlap of the two ranges, every source byte read before it is overwritten.  `workspace` is a
    DeviceBuffer or address of at least move_workspace_bytes(n) bytes of the same device; None makes one, waits for the call and
    raises if the pass gave up (move_status).  Otherwise move_status(workspace) tells the outcome after a synchronise."""
    if workspace is None:
        if not n:
            return
        ws = DeviceBuffer(move_workspace_bytes(n), device)
        try:
            rekey_move_device(dst, src, n, key_from, key_to, off_from, off_to, ws, device, stream)
            ws.sync(stream)
            stalled = move_status(ws, device)
            if stalled is not None:
                raise ModGpuError(3, f"the move gave up waiting at chunk {stalled}")
        finally:
            ws.free()
        return
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else move_workspace_bytes(n)
    _check(lib().modgpu_rekey_move_device(_vp(_dev_addr(dst)), _vp(_dev_addr(src)), n, as_int32(key_from), off_from, as_int32(key_to), off_to,
                                          _vp(_dev_addr(workspace)), ws_bytes, device, _vp(stream or 0)))


def move_status(workspace, device=-1):
    """None if the last rekey_move_device on `workspace` ran clean, else the chunk of the body whose wait ran out (the destination's
    contents are then unspecified).  Synchronise the call's stream first."""
    out = _u64(0)
    rc = lib().modgpu_move_status(_vp(_dev_addr(workspace)), device, ctypes.byref(out))
    if rc == 3 and out.value != (1 << 64) - 1:
        return int(out.value)
    _check(rc)
    return None


def debug_set_move_grid(grid=0):
    """Testing flavour: the grid of rekey_move_device's body launch (0 = shipped; capped at what the device holds at once)."""
    _debug_lib().modgpu_debug_set_move_grid(grid)


REKEY_FORMS = {None: -1, "shipped": -1, "queue": 0, "all": 1}


def debug_set_rekey_form(form=None):
    """Testing flavour: the rekey kernel's launch shape ("queue" = the out-of-place kernel's 200 workgroups, "all" = one per CU,
    None = shipped)."""
    _debug_lib().modgpu_debug_set_rekey_form(REKEY_FORMS[form])


def table(n):
    """an all-zero host table of n entries (TABLE_DTYPE): fill dst, src, n, stream_off, key; flags stay 0"""
    return np.zeros(n, dtype=TABLE_DTYPE)


def table_workspace_bytes(n_entries):
    """bytes of device workspace a table call over n_entries needs (0 for none, or above the limit)"""
    return lib().modgpu_table_workspace_bytes(n_entries)


def table_validate(entries):
    """the overlap / pointer / flags rules over a host table (TABLE_DTYPE array); raises ModGpuError naming an entry at fault"""
    t = np.ascontiguousarray(entries, dtype=TABLE_DTYPE)
    _check(lib().modgpu_table_validate(_vp(t.ctypes.data if t.size else 0), t.size))


def table_status(workspace, device=-1):
    """None if the last table call on `workspace` (a DeviceBuffer or address) ran clean, else the lowest entry the device refused
    (that call wrote nothing).  Synchronise the call's stream first."""
    out = _u64(0)
    rc = lib().modgpu_table_status(_vp(_dev_addr(workspace)), device, ctypes.byref(out))
    if rc == 1 and out.value != (1 << 64) - 1:
        return int(out.value)
    _check(rc)
    return None


def _no_verify_results():
    return np.zeros(0, dtype=VERIFY_RESULT_DTYPE)


def _no_digest_results():
    return np.zeros(0, dtype=DIGEST_RESULT_DTYPE), np.zeros(0, dtype=np.uint32)


def _table_call(call, entries, dtype, n, workspace, need, device, stream, refused, *, validate=None, needed="n (the entry count) is",
                known=True, extra=(), fetch=None, results=None, empty=None, status=table_status, gave_up=None, then=None):
    """Every *_table_device call: library function `call` gets (table, n, [results], *extra, workspace, its bytes, device, stream).
    The table `entries` is a host array of `dtype` -- checked with `validate`, uploaded; an empty one makes no call and returns
    empty(), or None -- or is in device memory already: then n is needed, and whatever else the caller says is `known`, and its
    address goes to the library as it is, which refuses a NULL one.  `results`, the buffer of 32-byte records, is an argument only of
    the calls that have a `fetch` (verify_results or digest_results); None makes one, as workspace=None makes one of need(n) bytes.
    When a buffer was made here the call is waited for, `status` is read -- table_status's one outcome, or rekey_move_table_status's
    pair -- and ModGpuError raised with the text `refused` (code 1) or `gave_up` (code 3); then the results are fetched and returned,
    and every buffer made here is freed, whatever happened.  Otherwise the call is asynchronous and None is returned.
    `then(res, n, ws, stv, own)`, for a table that was uploaded here, queues more work behind the call on the same stream -- the buffers
    it makes go into `own` -- and returns what reads that work's outcome once the stream has been waited for and the status was clean:
    the wrapper then returns the pair (what it returns without `then`, that outcome)."""
    own = []
    try:
        if isinstance(entries, np.ndarray):
            t = np.ascontiguousarray(entries, dtype=dtype)
            if validate:
                validate(t)
            if t.size == 0:
                return empty() if empty else None
            entries, n = DeviceBuffer(t.nbytes, device), t.size
            own.append(entries)
            entries.upload(t.view(np.uint8))
        elif n is None or not known:
            raise TypeError(f"{needed} needed for a table in device memory")
        if fetch and results is None and n:
            results = DeviceBuffer(n * 32, device)
            own.append(results)
        res = _dev_addr(results) if results is not None else 0
        if workspace is None and n:
            workspace = DeviceBuffer(need(n), device)
            own.append(workspace)
        ws = _dev_addr(workspace) if workspace is not None else 0
        ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else need(n)
        stv = _vp(stream or 0)
        _check(getattr(lib(), call)(_vp(_dev_addr(entries)), n, *((_vp(res),) if fetch else ()), *extra, _vp(ws), ws_bytes, device, stv))
        if not own:
            return None
        after = then(res, n, ws, stv, own) if then else None
        _check(lib().modgpu_sync(device, stv))
        outcome = status(ws, device)
        bad, stalled = outcome if isinstance(outcome, tuple) else (outcome, None)
        if bad is not None:
            raise ModGpuError(1, refused.format(bad))
        if stalled is not None:
            raise ModGpuError(3, gave_up.format(stalled))
        fetched = fetch(res, n, device) if fetch else None
        return (fetched, after()) if then else fetched
    finally:
        for b in own:
            b.free()


def _time_call(call, args, device, stream, iters):
    """Every time_* call: library function `call` with `args`, then device, stream, iters and the float it stores its mean ms in."""
    ms = ctypes.c_float(0)
    _check(getattr(lib(), call)(*args, device, _vp(stream or 0), iters, ctypes.byref(ms)))
    return ms.value


def cycle_table_device(entries, workspace=None, device=-1, stream=None, check=True, *, n=None):
    """Cycles a TABLE of out-of-place entries -- dst_i[j] = src_i[j] ^ ks(key_i)[stream_off_i + j] -- in three launches, whatever its
    length.  `entries` is a host table (a TABLE_DTYPE array: uploaded, and checked with table_validate first unless check=False) or a
    table already in device memory (a DeviceBuffer or an address; then n, the entry count, is needed).  `workspace` is a DeviceBuffer
    or address of at least table_workspace_bytes(n) bytes; None makes one.  When this function made a buffer itself (an uploaded
    table, a workspace) it waits for the call before freeing it and raises ModGpuError if the device refused an entry; otherwise the
    call is asynchronous on `stream` and table_status(workspace) tells the outcome after a synchronise."""
    _table_call("modgpu_cycle_table_device", entries, TABLE_DTYPE, n, workspace, table_workspace_bytes, device, stream,
                "the device refused table entry {}; nothing was written", validate=table_validate if check else None)


def time_cycle_table_device(entries, n, workspace, device=-1, stream=None, iters=2):
    """Mean ms per table call (three launches) over `iters` calls, HIP events on the launch stream; table and workspace resident."""
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else table_workspace_bytes(n)
    return _time_call("modgpu_time_cycle_table_device", (_vp(_dev_addr(entries)), n, _vp(_dev_addr(workspace)), ws_bytes), device, stream, iters)


def table_kernel_source_hash():
    """identity of the table kernels' TU (cycle_table_kernel.hip and what it includes)"""
    return lib().modgpu_table_kernel_source_hash().decode()


def debug_set_table_grid(grid=0):
    """Testing flavour: the table call's stream grid (0 = shipped)."""
    _debug_lib().modgpu_debug_set_table_grid(grid)


def rekey_table(n):
    """an all-zero host rekey table of n entries (REKEY_TABLE_DTYPE): fill dst, src, n, off_from, off_to, key_from, key_to; flags and
    reserved stay 0"""
    return np.zeros(n, dtype=REKEY_TABLE_DTYPE)


def rekey_table_workspace_bytes(n_entries):
    """bytes of device workspace a rekey table call over n_entries needs (0 for none, or above the limit)"""
    return lib().modgpu_rekey_table_workspace_bytes(n_entries)


def rekey_table_validate(entries):
    """the overlap / pointer / flags rules over a host rekey table (REKEY_TABLE_DTYPE array); raises ModGpuError naming an entry at
    fault"""
    t = np.ascontiguousarray(entries, dtype=REKEY_TABLE_DTYPE)
    _check(lib().modgpu_rekey_table_validate(_vp(t.ctypes.data if t.size else 0), t.size))


def rekey_table_device(entries, workspace=None, device=-1, stream=None, check=True, *, n=None):
    """Rekeys a TABLE of entries -- dst_i[j] = src_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j] -- in three
    launches, whatever its length.  `entries` is a host table (a REKEY_TABLE_DTYPE array: uploaded, and checked with
    rekey_table_validate first unless check=False) or a table already in device memory (a DeviceBuffer or an address; then n, the entry
    count, is needed).  `workspace` is a DeviceBuffer or address of at least rekey_table_workspace_bytes(n) bytes; None makes one.
    When this function made a buffer itself it waits for the call before freeing it and raises ModGpuError if the device refused an
    entry; otherwise the call is asynchronous on `stream` and table_status(workspace) tells the outcome after a synchronise."""
    _table_call("modgpu_rekey_table_device", entries, REKEY_TABLE_DTYPE, n, workspace, rekey_table_workspace_bytes, device, stream,
                "the device refused rekey table entry {}; nothing was written", validate=rekey_table_validate if check else None)


def time_rekey_table_device(entries, n, workspace, device=-1, stream=None, iters=2):
    """Mean ms per rekey table call (three launches) over `iters` calls, HIP events on the launch stream; table and workspace
    resident."""
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else rekey_table_workspace_bytes(n)
    return _time_call("modgpu_time_rekey_table_device", (_vp(_dev_addr(entries)), n, _vp(_dev_addr(workspace)), ws_bytes), device, stream, iters)


def rekey_table_kernel_source_hash():
    """identity of the rekey table kernels' TU (cycle_rekey_table_kernel.hip and what it includes)"""
    return lib().modgpu_rekey_table_kernel_source_hash().decode()


def debug_set_rekey_table_grid(grid=0):
    """Testing flavour: the rekey table call's stream grid (0 = shipped)."""
    _debug_lib().modgpu_debug_set_rekey_table_grid(grid)


def rekey_move_table_workspace_bytes(n_entries, total_bytes):
    """bytes of device workspace a rekey move table call needs for n_entries entries of at most total_bytes bytes together (0 for no
    entries, above the limit, or a total beyond 2^31 chunks)"""
    return lib().modgpu_rekey_move_table_workspace_bytes(n_entries, total_bytes)


def rekey_move_table_validate(entries):
    """the pointer / flags / direction / order rules of rekey_move_table_device over a host table (REKEY_TABLE_DTYPE array); raises
    ModGpuError naming an entry at fault"""
    t = np.ascontiguousarray(entries, dtype=REKEY_TABLE_DTYPE)
    _check(lib().modgpu_rekey_move_table_validate(_vp(t.ctypes.data if t.size else 0), t.size))


def rekey_move_table_status(workspace, device=-1):
    """(first_bad_entry, stalled_chunk) of the last rekey_move_table_device on `workspace`, each None when it does not apply: (None,
    None) if the call ran clean, (i, None) if the device refused entry i (the call wrote nothing), (None, c) if the wait of chunk c
    ran out (the destinations are then unspecified).  Synchronise the call's stream first."""
    bad, stalled = _u64(0), _u64(0)
    rc = lib().modgpu_rekey_move_table_status(_vp(_dev_addr(workspace)), device, ctypes.byref(bad), ctypes.byref(stalled))
    none = (1 << 64) - 1
    if rc == 1 and bad.value != none:
        return int(bad.value), None
    if rc == 3 and stalled.value != none:
        return None, int(stalled.value)
    _check(rc)
    return None, None


def rekey_move_table_device(entries, total_bytes=None, workspace=None, device=-1, stream=None, check=True, *, n=None):
    """Moves and rekeys a TABLE of entries with memmove rules -- dst_i[j] = SRC0_i[j] ^ ks(key_from_i)[off_from_i + j] ^
    ks(key_to_i)[off_to_i + j], every source byte of every entry read before any entry overwrites it -- in one pass, five launches
    whatever its length.  The table must be downward or upward (include/modgpu.h).  `entries` is a host table (a REKEY_TABLE_DTYPE
    array: uploaded, and checked with rekey_move_table_validate first unless check=False; total_bytes then defaults to the sum of its
    sizes) or a table already in device memory (a DeviceBuffer or an address; then n, the entry count, and total_bytes, an upper
    bound on the sum of the sizes, are needed).  `workspace` is a DeviceBuffer or address of at least
    rekey_move_table_workspace_bytes(n, total_bytes) bytes; None makes one.  When this function made a buffer itself it waits for the
    call before freeing it and raises ModGpuError if the device refused an entry or the pass gave up; otherwise the call is
    asynchronous on `stream` and rekey_move_table_status(workspace) tells the outcome after a synchronise."""
    known = total_bytes is not None
    if not known and isinstance(entries, np.ndarray):
        entries = np.ascontiguousarray(entries, dtype=REKEY_TABLE_DTYPE)
        total_bytes = int(entries["n"].sum(dtype=np.uint64))
    _table_call("modgpu_rekey_move_table_device", entries, REKEY_TABLE_DTYPE, n, workspace,
                lambda k: rekey_move_table_workspace_bytes(k, total_bytes), device, stream,
                "the device refused move table entry {}; nothing was written", gave_up="the move table pass gave up waiting at chunk {}",
                validate=rekey_move_table_validate if check else None, needed="n (the entry count) and total_bytes are", known=known,
                extra=(total_bytes,), status=rekey_move_table_status)


def compaction_table(base_ptr, keep, key, part_off=0):
    """The downward table that compacts a resident part: `keep` is a rising list of (offset, n) ranges of the part at device address
    base_ptr that survive; the result (REKEY_TABLE_DTYPE) packs them end to end from the first range's offset, under one key, with
    off_from = part_off + offset and off_to = part_off + the new offset."""
    keep = [(int(o), int(n)) for o, n in keep]
    t = rekey_table(len(keep))
    at = keep[0][0] if keep else 0
    for i, (o, n) in enumerate(keep):
        if o < at:
            raise ValueError(f"kept range {i} starts at {o}, below the end of the one before it ({at})")
        t[i]["dst"], t[i]["src"], t[i]["n"] = base_ptr + at, base_ptr + o, n
        t[i]["off_from"], t[i]["off_to"] = part_off + o, part_off + at
        t[i]["key_from"] = t[i]["key_to"] = as_int32(key)
        at += n
    return t


def rekey_relayout_table_validate(entries):
    """the pointer / flags / order rules of rekey_relayout_table_device over a host table (REKEY_TABLE_DTYPE array) -- the move table
    call's without the direction clause; raises ModGpuError naming an entry at fault"""
    t = np.ascontiguousarray(entries, dtype=REKEY_TABLE_DTYPE)
    _check(lib().modgpu_rekey_relayout_table_validate(_vp(t.ctypes.data if t.size else 0), t.size))


def rekey_relayout_table_device(entries, total_bytes=None, workspace=None, device=-1, stream=None, check=True, *, n=None):
    """rekey_move_table_device for a table whose entries slide BOTH ways -- listed by rising address, sources pairwise disjoint,
    destinations pairwise disjoint, no direction clause (include/modgpu.h) -- in one pass, ten launches whatever its length: the
    entries with dst <= src in a first sweep, those with dst > src in a second.  Arguments, workspace
    (rekey_move_table_workspace_bytes) and status (rekey_move_table_status) are rekey_move_table_device's; a host table is checked
    with rekey_relayout_table_validate first unless check=False."""
    known = total_bytes is not None
    if not known and isinstance(entries, np.ndarray):
        entries = np.ascontiguousarray(entries, dtype=REKEY_TABLE_DTYPE)
        total_bytes = int(entries["n"].sum(dtype=np.uint64))
    _table_call("modgpu_rekey_relayout_table_device", entries, REKEY_TABLE_DTYPE, n, workspace,
                lambda k: rekey_move_table_workspace_bytes(k, total_bytes), device, stream,
                "the device refused relayout table entry {}; nothing was written", gave_up="the relayout pass gave up waiting at chunk {}",
                validate=rekey_relayout_table_validate if check else None, needed="n (the entry count) and total_bytes are", known=known,
                extra=(total_bytes,), status=rekey_move_table_status)


def relayout_table(base_ptr, moves, key, key_to=None, part_off=0):
    """The table that relays out a resident part: `moves` is a list of (src_off, dst_off, n) segments of the part at device address
    base_ptr, rising and disjoint on both sides, sliding either way; the result (REKEY_TABLE_DTYPE) moves each from stream offset
    part_off + src_off under `key` to part_off + dst_off under key_to (None: `key`)."""
    moves = [(int(s), int(d), int(n)) for s, d, n in moves]
    t = rekey_table(len(moves))
    for i, (s, d, n) in enumerate(moves):
        t[i]["dst"], t[i]["src"], t[i]["n"] = base_ptr + d, base_ptr + s, n
        t[i]["off_from"], t[i]["off_to"] = part_off + s, part_off + d
        t[i]["key_from"], t[i]["key_to"] = as_int32(key), as_int32(key if key_to is None else key_to)
    return t


def splice_moves(size, edits):
    """The arithmetic of a splice: `edits` is a list of (offset, old_len, new_len) with rising, disjoint [offset, offset + old_len) inside
    a part of `size` bytes -- old_len bytes at offset give way to new_len bytes.  Returns (moves, new_size, holes): `moves` the
    surviving segments between the edits as (src_off, dst_off, n), each slid by the sum of the size changes before it (empty ones
    left out); `holes` the (new_offset, new_len) of every edit with new_len > 0, for the caller to fill.  ValueError on overlapping
    or falling edits, or one that passes the end of the part."""
    moves, holes = [], []
    at, shift = 0, 0  # the end of the last edit in the old part; new offset - old offset from there on
    for i, (off, old, new) in enumerate((int(o), int(a), int(b)) for o, a, b in edits):
        if off < at or old < 0 or new < 0 or off + old > size:
            raise ValueError(f"edit {i} ({off}, {old}, {new}) starts below the end of the one before it ({at}) or passes the part's size ({size})")
        if off > at:
            moves.append((at, at + shift, off - at))
        if new:
            holes.append((off + shift, new))
        shift += new - old
        at = off + old
    if size > at:
        moves.append((at, at + shift, size - at))
    return moves, size + shift, holes


def rekey_move_table_kernel_source_hash():
    """identity of the rekey move table kernels' TU (cycle_rekey_move_table_kernel.hip and what it includes)"""
    return lib().modgpu_rekey_move_table_kernel_source_hash().decode()


def debug_set_move_table_grid(grid=0):
    """Testing flavour: the grid of rekey_move_table_device's move launch (0 = shipped; capped at what the device holds at once)."""
    _debug_lib().modgpu_debug_set_move_table_grid(grid)


def verify_device(expect, src, key, stream_off=0, result=None, device=-1, stream=None, *, n=None):
    """Asynchronous VERIFY of n bytes at raw device addresses: counts the j with expect[j] != (src[j] ^ ks(key)[stream_off + j]) and
    finds the lowest, in one read-only pass; only the 32-byte result (device memory: a DeviceBuffer or an address) is written.
    `expect` / `src` are addresses or DeviceBuffer; n defaults to the smaller buffer's size when both are DeviceBuffer.  With
    result=None a result buffer is made, the stream synchronised and the result returned as a VERIFY_RESULT_DTYPE record."""
    r = _own_result_call("modgpu_verify_device", expect, src, n, (as_int32(key), stream_off), result, device, stream, verify_results)
    return r if r is None else r[0]


def verify_batch_device(expect_ptrs, src_ptrs, sizes, key, results, stream_offs=None, device=-1, stream=None):
    """Several verify entries of ONE device (entry i from stream_offs[i] or 0, its result at results + 32 * i); every range is only
    read, so anything may overlap anything.  One launch initialises the results, up to 16 non-empty entries share a compare launch."""
    n = len(expect_ptrs)
    assert len(src_ptrs) == n and len(sizes) == n
    _check(lib().modgpu_verify_batch_device(_ptr_array(expect_ptrs), _ptr_array(src_ptrs), _u64_array(sizes), _u64_array(stream_offs), n,
                                            as_int32(key), _vp(_dev_addr(results)), device, _vp(stream or 0)))


def verify_results(results, count=1, device=-1):
    """`count` results from device memory (a DeviceBuffer or an address) as a VERIFY_RESULT_DTYPE array; synchronous small copy --
    synchronise the stream the verify calls ran on first."""
    out = np.zeros(count, dtype=VERIFY_RESULT_DTYPE)
    _check(lib().modgpu_verify_results(_vp(_dev_addr(results)), count, device, _vp(out.ctypes.data if count else 0)))
    return out


def time_verify_device(expect, src, n, key, result, stream_off=0, device=-1, stream=None, iters=2):
    """Mean ms per verify call (two launches) over `iters` calls, HIP events on the launch stream."""
    return _time_call("modgpu_time_verify_device", (_vp(_dev_addr(expect)), _vp(_dev_addr(src)), n, as_int32(key), stream_off,
                                                    _vp(_dev_addr(result))), device, stream, iters)


def verify_kernel_source_hash():
    """identity of the verify kernels' TU (cycle_verify_kernel.hip and what it includes)"""
    return lib().modgpu_verify_kernel_source_hash().decode()


def debug_set_verify_form(grid=0):
    """Testing flavour: the most workgroups a verify compare launch takes (0 = shipped: one per CU)."""
    _debug_lib().modgpu_debug_set_verify_form(grid)


def digest_device(src, key, stream_off=0, dst=None, result=None, device=-1, stream=None, *, n=None):
    """Asynchronous DIGEST of n bytes at raw device addresses: the Adler-32 (zlib's) of out[j] = src[j] ^ ks(key)[stream_off + j] in one
    pass that reads n bytes; with `dst` the bytes are stored as cycle_device_to stores them and summed on the way (fused).  `src` /
    `dst` are addresses or DeviceBuffer; n defaults to the source's size (the smaller one's with a DeviceBuffer dst).  The 32-byte record
    `result` is device memory (a DeviceBuffer or an address).  With result=None a record is made, the stream synchronised and the
    Adler-32 returned as an int."""
    r = _own_result_call("modgpu_digest_device", dst, src, n, (as_int32(key), stream_off), result, device, stream, digest_results,
                         "the buffers are", True)
    return r if r is None else int(r[1][0])


def digest_batch_device(src_ptrs, sizes, key, results, dst_ptrs=None, stream_offs=None, device=-1, stream=None):
    """Several digest entries of ONE device (entry i from stream_offs[i] or 0, its record at results + 32 * i).  dst_ptrs None, or a None /
    0 entry: that entry is digest only.  One memset zeroes the records, up to 16 non-empty entries share a launch."""
    n = len(src_ptrs)
    assert len(sizes) == n and (dst_ptrs is None or len(dst_ptrs) == n)
    _check(lib().modgpu_digest_batch_device(_ptr_array(dst_ptrs), _ptr_array(src_ptrs), _u64_array(sizes), _u64_array(stream_offs), n,
                                            as_int32(key), _vp(_dev_addr(results)), device, _vp(stream or 0)))


def digest_results(results, count=1, device=-1):
    """`count` records from device memory (a DeviceBuffer or an address): (a DIGEST_RESULT_DTYPE array, their Adler-32 values as a uint32
    array); synchronous small copy -- synchronise the stream the digest calls ran on first."""
    out = np.zeros(count, dtype=DIGEST_RESULT_DTYPE)
    adler = np.zeros(count, dtype=np.uint32)
    _check(lib().modgpu_digest_results(_vp(_dev_addr(results)), count, device, _vp(out.ctypes.data if count else 0),
                                       adler.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if count else None))
    return out, adler


def digest_adler32(record):
    """Adler-32 from one record in host memory (a DIGEST_RESULT_DTYPE scalar or a (s1, s2, n) tuple); pure arithmetic in the library."""
    r = np.zeros(1, dtype=DIGEST_RESULT_DTYPE)
    if isinstance(record, (tuple, list)):
        r["s1"], r["s2"], r["n"] = record[:3]
    else:
        r[0] = record
    return int(lib().modgpu_digest_adler32(_vp(r.ctypes.data)))


def time_digest_device(src, n, key, result, dst=None, stream_off=0, device=-1, stream=None, iters=2):
    """Mean ms per digest call (the memset node and one launch) over `iters` calls, HIP events on the launch stream."""
    return _time_call("modgpu_time_digest_device", (_vp(_dev_addr(dst) if dst is not None else 0), _vp(_dev_addr(src)), n, as_int32(key), stream_off,
                                                    _vp(_dev_addr(result))), device, stream, iters)


def debug_set_digest_grid(grid=0):
    """Testing flavour: the most workgroups a digest launch takes (0 = shipped: one per CU).  Every grid gives the same sums."""
    _debug_lib().modgpu_debug_set_digest_grid(grid)


def verify_rekey_device(expect, src, key_from, key_to, off_from=0, off_to=0, result=None, device=-1, stream=None, *, n=None):
    """Asynchronous REKEY VERIFY of n bytes at raw device addresses: counts the j with expect[j] != (src[j] ^ ks(key_from)[off_from + j]
    ^ ks(key_to)[off_to + j]) -- the bytes rekey_device_to would have written -- and finds the lowest, in one read-only pass; only the
    32-byte result (device memory: a DeviceBuffer or an address) is written.  Arguments and the result=None convenience as
    verify_device."""
    r = _own_result_call("modgpu_verify_rekey_device", expect, src, n, (as_int32(key_from), off_from, as_int32(key_to), off_to), result, device,
                         stream, verify_results)
    return r if r is None else r[0]


def verify_rekey_batch_device(expect_ptrs, src_ptrs, sizes, key_from, key_to, results, offs_from=None, offs_to=None, device=-1, stream=None):
    """Several rekey verify entries of ONE device under one pair of keys (entry i at offs_from[i] / offs_to[i] or 0, its result at
    results + 32 * i); every range is only read, so anything may overlap anything.  One launch initialises the results, up to 16
    non-empty entries whose two streams differ share a compare launch, and so do up to 16 whose streams coincide."""
    n = len(expect_ptrs)
    assert len(src_ptrs) == n and len(sizes) == n
    _check(lib().modgpu_verify_rekey_batch_device(_ptr_array(expect_ptrs), _ptr_array(src_ptrs), _u64_array(sizes), _u64_array(offs_from),
                                                  _u64_array(offs_to), n, as_int32(key_from), as_int32(key_to), _vp(_dev_addr(results)),
                                                  device, _vp(stream or 0)))


def time_verify_rekey_device(expect, src, n, key_from, key_to, result, off_from=0, off_to=0, device=-1, stream=None, iters=2):
    """Mean ms per rekey verify call (two launches) over `iters` calls, HIP events on the launch stream."""
    return _time_call("modgpu_time_verify_rekey_device", (_vp(_dev_addr(expect)), _vp(_dev_addr(src)), n, as_int32(key_from), off_from,
                                                          as_int32(key_to), off_to, _vp(_dev_addr(result))), device, stream, iters)


def keep_kernel_source_hash():
    """SHA-256 over the keep kernel's TU (the work-queue kernel with a resident slice; include/modgpu_testing.h)."""
    return lib().modgpu_keep_kernel_source_hash().decode()


KEEP_OFF = (1 << 64) - 1


def keep_policy(nbytes):
    """(takes the keep kernel?, mask, run) of a single in-place device buffer of `nbytes` bytes (modgpu_keep_policy)."""
    mask, run = ctypes.c_uint32(), ctypes.c_uint32()
    route = lib().modgpu_keep_policy(nbytes, ctypes.byref(mask), ctypes.byref(run))
    return bool(route), mask.value, run.value


def debug_set_keep(min_bytes=0, mask=0, run=0):
    """Test / measurement hook: single-buffer work-queue launches of `min_bytes` or more take the keep kernel with this (mask, run);
    KEEP_OFF switches the route off; (0, 0, 0) restores the shipped rule."""
    _debug_lib().modgpu_debug_set_keep(min_bytes, mask, run)


def rekey_verify_kernel_source_hash():
    """identity of the rekey verify kernel's TU (cycle_rekey_verify_kernel.hip and what it includes)"""
    return lib().modgpu_rekey_verify_kernel_source_hash().decode()


def verify_table_workspace_bytes(n_entries):
    """bytes of device workspace a verify table call over n_entries needs (0 for none, or above the limit)"""
    return lib().modgpu_verify_table_workspace_bytes(n_entries)


def verify_table_summary(workspace, device=-1):
    """The last verify table call on `workspace` (a DeviceBuffer or address) as a dict: mismatches (all entries' sum), first_bad_entry
    (the lowest entry with a mismatch, None if there is none), entries.  Synchronise the call's stream first.  Raises ModGpuError if
    the device refused the call (table_status names the entry)."""
    out = np.zeros(1, dtype=VERIFY_TABLE_SUMMARY_DTYPE)
    _check(lib().modgpu_verify_table_summary(_vp(_dev_addr(workspace)), device, _vp(out.ctypes.data)))
    first = int(out["first_bad_entry"][0])
    return {"mismatches": int(out["mismatches"][0]), "first_bad_entry": None if first == VERIFY_NONE else first, "entries": int(out["entries"][0])}


def verify_table_device(entries, results=None, workspace=None, device=-1, stream=None, *, n=None):
    """VERIFIES a TABLE of entries in three launches, whatever its length: for entry i the count of the j with dst_i[j] !=
    (src_i[j] ^ ks(key_i)[stream_off_i + j]) and the lowest such j -- `dst` is the comparand, nothing but the results and the workspace
    is written, anything may overlap anything.  `entries` is a host table (a TABLE_DTYPE array: uploaded) or a table already in device
    memory (a DeviceBuffer or an address; then n, the entry count, is needed).  `results` is a DeviceBuffer or address of 32 * n bytes,
    `workspace` one of at least verify_table_workspace_bytes(n) bytes; None makes one.  When this function made a buffer itself it
    waits for the call, raises ModGpuError if the device refused an entry (no result was written) and returns the results as a
    VERIFY_RESULT_DTYPE array; otherwise the call is asynchronous on `stream`, returns None, and table_status(workspace),
    verify_table_summary(workspace) and verify_results(results, n) tell the outcome after a synchronise."""
    return _table_call("modgpu_verify_table_device", entries, TABLE_DTYPE, n, workspace, verify_table_workspace_bytes, device, stream,
                       "the device refused verify table entry {}; no result was written", fetch=verify_results, results=results,
                       empty=_no_verify_results)


def time_verify_table_device(entries, n, results, workspace, device=-1, stream=None, iters=2):
    """Mean ms per verify table call (three launches) over `iters` calls, HIP events on the launch stream; table, results and
    workspace resident."""
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else verify_table_workspace_bytes(n)
    return _time_call("modgpu_time_verify_table_device", (_vp(_dev_addr(entries)), n, _vp(_dev_addr(results)), _vp(_dev_addr(workspace)), ws_bytes), device,
                      stream, iters)


def verify_table_kernel_source_hash():
    """identity of the verify table kernels' TU (cycle_verify_table_kernel.hip and what it includes)"""
    return lib().modgpu_verify_table_kernel_source_hash().decode()


def debug_set_verify_table_grid(grid=0):
    """Testing flavour: the verify table call's stream grid (0 = shipped)."""
    _debug_lib().modgpu_debug_set_verify_table_grid(grid)


def digest_table_workspace_bytes(n_entries):
    """bytes of device workspace a digest table call over n_entries needs (0 for none, or above the limit): table_workspace_bytes(n)"""
    return lib().modgpu_digest_table_workspace_bytes(n_entries)


def digest_table_device(entries, results=None, workspace=None, device=-1, stream=None, *, n=None):
    """DIGESTS a TABLE of entries in three launches, whatever its length: for entry i the record of out[j] = src_i[j] ^
    ks(key_i)[stream_off_i + j] -- `dst` of an entry is ignored, nothing but the records and the workspace is written, anything may
    overlap anything.  `entries` is a host table (a TABLE_DTYPE array: uploaded) or a table already in device memory (a DeviceBuffer or
    an address; then n, the entry count, is needed).  `results` is a DeviceBuffer or address of 32 * n bytes, `workspace` one of at
    least digest_table_workspace_bytes(n) bytes; None makes one.  When this function made a buffer itself it waits for the call, raises
    ModGpuError if the device refused an entry (no record was written) and returns (the records as a DIGEST_RESULT_DTYPE array, their
    Adler-32 values as a uint32 array); otherwise the call is asynchronous on `stream`, returns None, and table_status(workspace) and
    digest_results(results, n) tell the outcome after a synchronise."""
    return _table_call("modgpu_digest_table_device", entries, TABLE_DTYPE, n, workspace, digest_table_workspace_bytes, device, stream,
                       "the device refused digest table entry {}; no record was written", fetch=digest_results, results=results,
                       empty=_no_digest_results)


def time_digest_table_device(entries, n, results, workspace, device=-1, stream=None, iters=2):
    """Mean ms per digest table call (three launches) over `iters` calls, HIP events on the launch stream; table, records and
    workspace resident."""
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else digest_table_workspace_bytes(n)
    return _time_call("modgpu_time_digest_table_device", (_vp(_dev_addr(entries)), n, _vp(_dev_addr(results)), _vp(_dev_addr(workspace)), ws_bytes), device,
                      stream, iters)


def debug_set_digest_table_grid(grid=0):
    """Testing flavour: the digest table call's stream grid (0 = shipped: one workgroup per CU).  Every grid gives the same residues."""
    _debug_lib().modgpu_debug_set_digest_table_grid(grid)


def cycle_digest_table_workspace_bytes(n_entries):
    """bytes of device workspace a cycle digest table call over n_entries needs (0 for none, or above the limit): table_workspace_bytes(n)"""
    return lib().modgpu_cycle_digest_table_workspace_bytes(n_entries)


def cycle_digest_table_device(entries, records=None, side=DIGEST_OUTPUT, workspace=None, device=-1, stream=None, *, n=None):
    """Cycles a TABLE of out-of-place entries as cycle_table_device does AND digests every entry in the same pass, three launches
    whatever the length: record i is of what was stored (side=DIGEST_OUTPUT) or of the source bytes as read (DIGEST_INPUT).  `entries`
    is a host table (a TABLE_DTYPE array: uploaded) or a table already in device memory (a DeviceBuffer or an address; then n, the
    entry count, is needed).  `records` is a DeviceBuffer or address of 32 * n bytes, `workspace` one of at least
    cycle_digest_table_workspace_bytes(n) bytes; None makes one.  When this function made a buffer itself it waits for the call, raises
    ModGpuError if the device refused an entry (nothing was written, no byte and no record) and returns (the records as a
    DIGEST_RESULT_DTYPE array, their Adler-32 values as a uint32 array); otherwise the call is asynchronous on `stream`, returns None,
    and table_status(workspace) and digest_results(records, n) tell the outcome after a synchronise."""
    return _table_call("modgpu_cycle_digest_table_device", entries, TABLE_DTYPE, n, workspace, cycle_digest_table_workspace_bytes, device,
                       stream, "the device refused cycle digest table entry {}; nothing was written", extra=(side,), fetch=digest_results,
                       results=records, empty=_no_digest_results)


def time_cycle_digest_table_device(entries, n, records, workspace, side=DIGEST_OUTPUT, device=-1, stream=None, iters=2):
    """Mean ms per cycle digest table call (three launches) over `iters` calls, HIP events on the launch stream; table, records and
    workspace resident."""
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else cycle_digest_table_workspace_bytes(n)
    return _time_call("modgpu_time_cycle_digest_table_device", (_vp(_dev_addr(entries)), n, _vp(_dev_addr(records)), side, _vp(_dev_addr(workspace)),
                                                                ws_bytes), device, stream, iters)


def debug_set_cycle_digest_table_grid(grid=0):
    """Testing flavour: the cycle digest table call's stream grid (0 = shipped).  Every grid gives the same bytes and residues."""
    _debug_lib().modgpu_debug_set_cycle_digest_table_grid(grid)


def rekey_digest_table_workspace_bytes(n_entries):
    """bytes of device workspace a rekey digest table call over n_entries needs (0 for none, or above the limit):
    rekey_table_workspace_bytes(n)"""
    return lib().modgpu_rekey_digest_table_workspace_bytes(n_entries)


def rekey_digest_table_device(entries, records=None, side=DIGEST_PLAIN, workspace=None, device=-1, stream=None, *, n=None):
    """Rekeys a TABLE of rekey entries as rekey_table_device does AND digests every entry in the same pass, three launches whatever the
    length: record i is of src ^ ks(key_from), the plaintext between the two keystreams (side=DIGEST_PLAIN), of what was stored
    (DIGEST_OUTPUT) or of the source bytes as read (DIGEST_INPUT).  `entries` is a host table (a REKEY_TABLE_DTYPE array: uploaded) or a
    table already in device memory (a DeviceBuffer or an address; then n, the entry count, is needed).  `records` is a DeviceBuffer or
    address of 32 * n bytes, `workspace` one of at least rekey_digest_table_workspace_bytes(n) bytes; None makes one.  When this function
    made a buffer itself it waits for the call, raises ModGpuError if the device refused an entry (nothing was written, no byte and no
    record) and returns (the records as a DIGEST_RESULT_DTYPE array, their Adler-32 values as a uint32 array); otherwise the call is
    asynchronous on `stream`, returns None, and table_status(workspace) and digest_results(records, n) tell the outcome after a
    synchronise."""
    return _table_call("modgpu_rekey_digest_table_device", entries, REKEY_TABLE_DTYPE, n, workspace, rekey_digest_table_workspace_bytes, device,
                       stream, "the device refused rekey digest table entry {}; nothing was written", extra=(side,), fetch=digest_results,
                       results=records, empty=_no_digest_results)


def time_rekey_digest_table_device(entries, n, records, workspace, side=DIGEST_PLAIN, device=-1, stream=None, iters=2):
    """Mean ms per rekey digest table call (three launches) over `iters` calls, HIP events on the launch stream; table, records and
    workspace resident."""
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else rekey_digest_table_workspace_bytes(n)
    return _time_call("modgpu_time_rekey_digest_table_device", (_vp(_dev_addr(entries)), n, _vp(_dev_addr(records)), side, _vp(_dev_addr(workspace)),
                                                                ws_bytes), device, stream, iters)


def debug_set_rekey_digest_table_grid(grid=0):
    """Testing flavour: the rekey digest table call's stream grid (0 = shipped).  Every grid gives the same bytes and residues."""
    _debug_lib().modgpu_debug_set_rekey_digest_table_grid(grid)


def digest_check_bits_bytes(n_entries):
    """bytes of a digest check's bitmap over n_entries: 8 * ceil(n / 64) (0 for none, or above the table calls' limit)"""
    return lib().modgpu_digest_check_bits_bytes(n_entries)


def _no_bad_entries():
    return 0, None, np.zeros(0, dtype=np.uint64)


def digest_check_result(summary, n, bad_bits=None, device=-1):
    """What a digest check left in `summary` (and `bad_bits`; DeviceBuffer or address each): (bad entries, the lowest bad entry or
    None, the bad indices as a uint64 array -- None without a bitmap).  Synchronous small copies (32 bytes, and n / 8 only if an entry
    is bad): synchronise the stream the check ran on first.  Raises ModGpuError if the table call that produced the records had been
    refused (nothing was compared)."""
    out = np.zeros(1, dtype=DIGEST_CHECK_SUMMARY_DTYPE)
    _check(lib().modgpu_digest_check_summary(_vp(_dev_addr(summary)), device, _vp(out.ctypes.data)))
    bad, first = int(out["bad_entries"][0]), int(out["first_bad_entry"][0])
    if bad_bits is None:
        return bad, None if first == VERIFY_NONE else first, None
    if not bad:
        return _no_bad_entries()
    words = np.zeros((n + 63) // 64, dtype="<u8")
    _check(lib().modgpu_d2h(_vp(words.ctypes.data), _vp(_dev_addr(bad_bits)), words.nbytes, device))
    return bad, first, np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[:n]).astype(np.uint64)


def _queue_digest_check(records, expect, n, table_workspace, summary, bad_bits, device, stv, own):
    """One modgpu_digest_check_device call queued on stream `stv`; a host manifest is uploaded, and a missing bitmap made, into
    buffers appended to `own` (the caller frees them).  Returns the bitmap."""
    if isinstance(expect, np.ndarray):
        e = np.ascontiguousarray(expect, dtype=np.uint32)
        if e.size < n:
            raise ValueError(f"a manifest of {e.size} values for {n} entries")
        expect = DeviceBuffer(max(4 * n, 4), device)
        own.append(expect)
        expect.upload(e[:n].view(np.uint8))
    if bad_bits is None:
        bad_bits = DeviceBuffer(max(digest_check_bits_bytes(n), 8), device)
        own.append(bad_bits)
    _check(lib().modgpu_digest_check_device(_vp(_dev_addr(records)), _vp(_dev_addr(expect)), n,
                                            _vp(_dev_addr(table_workspace) if table_workspace is not None else 0), _vp(_dev_addr(summary)),
                                            _vp(_dev_addr(bad_bits)), device, stv))
    return bad_bits


def digest_check_device(records, expect, n, table_workspace=None, summary=None, bad_bits=None, device=-1, stream=None):
    """CHECKS n digest records in device memory (a DeviceBuffer or an address: what digest_device, digest_batch_device,
    digest_table_device or cycle_digest_table_device left there) against a manifest of Adler-32 values, on the device, in two
    launches: entry i is bad when its record does not close to expect[i].  `expect` is a device address, a DeviceBuffer or a host
    uint32 array (uploaded).  `table_workspace`, when given, is the workspace of the table call that produced the records: had the
    device refused that call nothing is compared and ModGpuError is raised.  `summary` (32 bytes) and `bad_bits`
    (digest_check_bits_bytes(n) bytes) are device memory.  With summary=None one is made (and a bitmap, unless given), the stream
    synchronised and (bad entries, the lowest bad entry or None, the bad indices as a uint64 array) returned after reading back 32
    bytes, and n / 8 more only if an entry is bad.  With a summary of the caller's the call is asynchronous on `stream` -- it can be
    captured into a graph --, returns None, and digest_check_result(summary, n, bad_bits) tells the outcome after a synchronise; no
    bitmap is written unless one is given."""
    if not n:
        return _no_bad_entries() if summary is None else None
    stv = _vp(stream or 0)
    own = []
    try:
        if summary is not None:
            if isinstance(expect, np.ndarray):
                raise TypeError("an asynchronous check needs its manifest in device memory")
            _check(lib().modgpu_digest_check_device(_vp(_dev_addr(records)), _vp(_dev_addr(expect)), n,
                                                    _vp(_dev_addr(table_workspace) if table_workspace is not None else 0), _vp(_dev_addr(summary)),
                                                    _vp(_dev_addr(bad_bits) if bad_bits is not None else 0), device, stv))
            return None
        summary = DeviceBuffer(32, device)
        own.append(summary)
        bad_bits = _queue_digest_check(records, expect, n, table_workspace, summary, bad_bits, device, stv, own)
        _check(lib().modgpu_sync(device, stv))
        return digest_check_result(summary, n, bad_bits, device)
    finally:
        for b in own:
            b.free()


def time_digest_check_device(records, expect, n, summary, bad_bits=None, table_workspace=None, device=-1, stream=None, iters=2):
    """Mean ms per digest check (two launches) over `iters` calls, HIP events on the launch stream; everything resident."""
    return _time_call("modgpu_time_digest_check_device", (_vp(_dev_addr(records)), _vp(_dev_addr(expect)), n,
                                                          _vp(_dev_addr(table_workspace) if table_workspace is not None else 0), _vp(_dev_addr(summary)),
                                                          _vp(_dev_addr(bad_bits) if bad_bits is not None else 0)), device, stream, iters)


def _check_behind(expect, device):
    """`then` of a digest producing table call (_table_call): a digest check of its records against `expect`, queued behind it"""
    def then(res, n, ws, stv, own):
        summary = DeviceBuffer(32, device)
        own.append(summary)
        bad_bits = _queue_digest_check(res, expect, n, ws, summary, None, device, stv, own)
        return lambda: digest_check_result(summary, n, bad_bits, device)
    return then


def _keep_on_device(res, n, device):
    """the `fetch` of a table call whose records stay where they are"""
    return None


def verify_rekey_table_workspace_bytes(n_entries):
    """bytes of device workspace a rekey verify table call over n_entries needs (0 for none, or above the limit)"""
    return lib().modgpu_verify_rekey_table_workspace_bytes(n_entries)


def verify_rekey_table_device(entries, results=None, workspace=None, device=-1, stream=None, *, n=None):
    """VERIFIES a TABLE of rekey entries in three launches, whatever its length: for entry i the count of the j with dst_i[j] !=
    (src_i[j] ^ ks(key_from_i)[off_from_i + j] ^ ks(key_to_i)[off_to_i + j]) and the lowest such j -- `dst` is the comparand, nothing
    but the results and the workspace is written, anything may overlap anything.  `entries` is a host table (a REKEY_TABLE_DTYPE array
    from rekey_table(n): uploaded) or a table already in device memory (a DeviceBuffer or an address; then n, the entry count, is
    needed).  `results` is a DeviceBuffer or address of 32 * n bytes, `workspace` one of at least verify_rekey_table_workspace_bytes(n)
    bytes; None makes one.  When this function made a buffer itself it waits for the call, raises ModGpuError if the device refused an
    entry (no result was written) and returns the results as a VERIFY_RESULT_DTYPE array; otherwise the call is asynchronous on
    `stream`, returns None, and table_status(workspace), verify_table_summary(workspace) and verify_results(results, n) tell the
    outcome after a synchronise."""
    return _table_call("modgpu_verify_rekey_table_device", entries, REKEY_TABLE_DTYPE, n, workspace, verify_rekey_table_workspace_bytes,
                       device, stream, "the device refused rekey verify table entry {}; no result was written", fetch=verify_results,
                       results=results, empty=_no_verify_results)


def time_verify_rekey_table_device(entries, n, results, workspace, device=-1, stream=None, iters=2):
    """Mean ms per rekey verify table call (three launches) over `iters` calls, HIP events on the launch stream; table, results and
    workspace resident."""
    ws_bytes = workspace.nbytes if isinstance(workspace, DeviceBuffer) else verify_rekey_table_workspace_bytes(n)
    return _time_call("modgpu_time_verify_rekey_table_device", (_vp(_dev_addr(entries)), n, _vp(_dev_addr(results)), _vp(_dev_addr(workspace)), ws_bytes), device,
                      stream, iters)


def rekey_verify_table_kernel_source_hash():
    """identity of the rekey verify table kernels' TU (cycle_rekey_verify_table_kernel.hip and what it includes)"""
    return lib().modgpu_rekey_verify_table_kernel_source_hash().decode()


def debug_set_rekey_verify_table_grid(grid=0):
    """Testing flavour: the rekey verify table call's stream grid (0 = shipped)."""
    _debug_lib().modgpu_debug_set_rekey_verify_table_grid(grid)


def _dev_addr(x):
    """raw device address of an int address or a DeviceBuffer"""
    return x.ptr if isinstance(x, DeviceBuffer) else x


TO_FORMS = {None: -1, "shipped": -1, "unaligned": 0, "funnel": 1}


def debug_set_to_form(form=None):
    """Testing flavour: how the out-of-place kernel reads a misaligned source ("unaligned" loads / "funnel" / None = shipped)."""
    _debug_lib().modgpu_debug_set_to_form(TO_FORMS[form])


def _xfer_src(buf):
    """(address, bytes) of a transfer's host SOURCE: a PinnedBuffer, a C-contiguous ndarray (read-only is fine) or a bytes-like object"""
    if isinstance(buf, PinnedBuffer):
        return buf.ptr, buf.nbytes
    if not isinstance(buf, np.ndarray):
        buf = np.frombuffer(buf, dtype=np.uint8)
    if not buf.flags["C_CONTIGUOUS"]:
        raise TypeError("need a C-contiguous buffer")
    return buf.ctypes.data, buf.nbytes


def _xfer_dst(buf):
    """(address, bytes) of a transfer's host DESTINATION: a PinnedBuffer or a writable C-contiguous ndarray"""
    if isinstance(buf, PinnedBuffer):
        return buf.ptr, buf.nbytes
    if not (isinstance(buf, np.ndarray) and buf.flags["C_CONTIGUOUS"] and buf.flags["WRITEABLE"]):
        raise TypeError("need a writable C-contiguous ndarray or a PinnedBuffer")
    return buf.ctypes.data, buf.nbytes


def cycle_host_to_device(dev_ptr, buf, key, stream_off=0, device=-1):
    """Upload with the cipher in flight: dev[j] = buf[j] ^ ks[stream_off + j] for every byte of `buf`; `buf` is not modified.
    Synchronous, and not ordered against the caller's streams (synchronise first)."""
    p, n = _xfer_src(buf)
    _check(lib().modgpu_cycle_host_to_device(_vp(dev_ptr), _vp(p), n, as_int32(key), stream_off, device))


def cycle_device_to_host(buf, dev_ptr, key, stream_off=0, device=-1):
    """Download with the cipher in flight: buf[j] = dev[j] ^ ks[stream_off + j] for every byte of `buf`; the device bytes are not
    modified.  Returns `buf`."""
    p, n = _xfer_dst(buf)
    _check(lib().modgpu_cycle_device_to_host(_vp(p), _vp(dev_ptr), n, as_int32(key), stream_off, device))
    return buf


def cycle_file_to_device(path, dev_ptr, n, key, file_off=0, stream_off=0, device=-1):
    """n bytes at file_off of a part file through the cipher into device memory."""
    _check(lib().modgpu_cycle_file_to_device(os.fsencode(path), file_off, _vp(dev_ptr), n, as_int32(key), stream_off, device))


def cycle_device_to_file(dev_ptr, n, path, key, stream_off=0, device=-1):
    """n device bytes through the cipher into `path` (created / truncated)."""
    _check(lib().modgpu_cycle_device_to_file(_vp(dev_ptr), n, os.fsencode(path), as_int32(key), stream_off, device))


def _xfer_list_table(entries, upload):
    """(table, arrays to keep alive) of a list transfer: `entries` is a host table (TABLE_DTYPE array, taken as it stands) or a list of
    (dev_ptr, array, key, stream_off) -- the array the host side of the entry, its source in an upload, its destination in a download"""
    if isinstance(entries, np.ndarray):
        return np.ascontiguousarray(entries, dtype=TABLE_DTYPE), ()
    entries = list(entries)
    t, keep = table(len(entries)), []
    for i, (dev_ptr, buf, key, stream_off) in enumerate(entries):
        p, n = _xfer_src(buf) if upload else _xfer_dst(buf)
        keep.append(buf)
        t[i]["dst"], t[i]["src"] = (_dev_addr(dev_ptr), p) if upload else (p, _dev_addr(dev_ptr))
        t[i]["n"], t[i]["stream_off"], t[i]["key"] = n, stream_off, as_int32(key)
    return t, keep


def cycle_host_to_device_list(entries, device=-1, check=False):
    """Upload of a list of ranges with the cipher in flight, ONE launch whatever the count (modgpu_cycle_host_to_device_list): for every
    entry dev[j] = host[j] ^ ks(key)[stream_off + j].  `entries` is a host table (TABLE_DTYPE: dst the device side, src the host side) or
    a list of (dev_ptr, array, key, stream_off).  check=True runs table_validate over the table first (the device destinations may not
    meet each other; the call itself does not look).  Synchronous, and not ordered against the caller's streams (synchronise first)."""
    t, keep = _xfer_list_table(entries, True)
    if check:
        table_validate(t)
    _check(lib().modgpu_cycle_host_to_device_list(_vp(t.ctypes.data if t.size else 0), t.size, device))
    del keep


def cycle_device_to_host_list(entries, device=-1, check=False):
    """Download of a list of ranges with the cipher in flight, ONE launch whatever the count (modgpu_cycle_device_to_host_list): for every
    entry host[j] = dev[j] ^ ks(key)[stream_off + j].  `entries` is a host table (TABLE_DTYPE: dst the host side, src the device side) or
    a list of (dev_ptr, array, key, stream_off), the arrays writable.  check=True runs table_validate over the table first (the host
    destinations may not meet each other)."""
    t, keep = _xfer_list_table(entries, False)
    if check:
        table_validate(t)
    _check(lib().modgpu_cycle_device_to_host_list(_vp(t.ctypes.data if t.size else 0), t.size, device))
    del keep


def _xfer_list_digest(name, entries, upload, side, records, device, check):
    """a digesting list transfer: (the records as a DIGEST_RESULT_DTYPE array, their Adler-32 values as a uint32 array)"""
    t, keep = _xfer_list_table(entries, upload)
    if check:
        table_validate(t)
    if not t.size:
        return _no_digest_results()
    own = None
    try:
        if records is None:
            records = own = DeviceBuffer(DIGEST_RESULT_DTYPE.itemsize * t.size, device)
        _check(getattr(lib(), name)(_vp(t.ctypes.data), t.size, side, _vp(_dev_addr(records)), device))
        return digest_results(records, t.size, device)
    finally:
        del keep
        if own is not None:
            own.free()


def cycle_host_to_device_list_digest(entries, side=DIGEST_OUTPUT, records=None, device=-1, check=False):
    """cycle_host_to_device_list with one digest record per entry, taken in the same launch (modgpu_cycle_host_to_device_list_digest):
    record i is of what was stored in entry i's device range (side=DIGEST_OUTPUT) or of its host bytes as read (DIGEST_INPUT: a packer's
    plaintext checksums while the ciphertext goes up).  `records` is device memory of 32 bytes per entry (a DeviceBuffer or an address;
    it then holds the records afterwards, for digest_check_device); None: a buffer is made and freed.  Returns (the records as a
    DIGEST_RESULT_DTYPE array, their Adler-32 values as a uint32 array)."""
    return _xfer_list_digest("modgpu_cycle_host_to_device_list_digest", entries, True, side, records, device, check)


def cycle_device_to_host_list_digest(entries, side=DIGEST_OUTPUT, records=None, device=-1, check=False):
    """cycle_device_to_host_list with one digest record per entry, taken in the same launch (modgpu_cycle_device_to_host_list_digest):
    record i is of what was stored in entry i's host array (side=DIGEST_OUTPUT: an extractor's plaintext checksums) or of its device
    bytes as read (DIGEST_INPUT).  `records` and the return value as cycle_host_to_device_list_digest has them."""
    return _xfer_list_digest("modgpu_cycle_device_to_host_list_digest", entries, False, side, records, device, check)


XFER_FORMS = {None: 0, "kernel": 0, "dma": 1}


def debug_set_xfer_form(form=None):
    """Testing flavour: how the transfer calls move their bytes ("kernel" = the transfer kernels, shipped; "dma" = the reference form)."""
    _debug_lib().modgpu_debug_set_xfer_form(XFER_FORMS[form])


def state_at(key, i):
    return lib().modgpu_state_at(as_int32(key), i)


def jump_table(which):
    out = (ctypes.c_uint32 * 256)()
    n = lib().modgpu_jump_table(which, out, 256)
    return list(out[:n])


class DeviceBuffer:
    """hipMalloc'd bytes owned through modgpu_alloc / modgpu_free."""

    def __init__(self, nbytes, device=-1):
        self.nbytes, self.device = nbytes, device
        p = _vp()
        self._lib = lib()
        _check(self._lib.modgpu_alloc(ctypes.byref(p), nbytes, device))
        self.ptr = p.value

    def upload(self, host, offset=0):
        host = np.ascontiguousarray(host, dtype=np.uint8)
        assert offset + host.size <= self.nbytes
        _check(self._lib.modgpu_h2d(_vp(self.ptr + offset), _vp(host.ctypes.data), host.size, self.device))

    def download(self, n=None, offset=0):
        n = self.nbytes - offset if n is None else n
        out = np.empty(n, dtype=np.uint8)
        _check(self._lib.modgpu_d2h(_vp(out.ctypes.data), _vp(self.ptr + offset), n, self.device))
        return out

    def cycle(self, key, n=None, offset=0, stream_off=0, stream=None):
        n = self.nbytes - offset if n is None else n
        assert offset + n <= self.nbytes
        cycle_device(self.ptr + offset, n, key, stream_off, self.device, stream)

    def digest(self, key, n=None, offset=0, stream_off=0, stream=None):
        """Adler-32 of what the cipher makes of n bytes from `offset` (digest_device, digest only): an int, after a synchronise."""
        n = self.nbytes - offset if n is None else n
        assert offset + n <= self.nbytes
        return digest_device(self.ptr + offset, key, stream_off, None, None, self.device, stream, n=n)

    def digests(self, ranges, key, part_off=0, workspace=None, stream=None):
        """One Adler-32 per range of `ranges` -- a list of (offset, n) -- of the part this buffer holds, each taken from stream offset
        part_off + offset, in one digest_table_device call: a uint32 array.  The read-only sibling of compact: "are these files of
        the part still the files I packed?"."""
        ranges = [(int(o), int(n)) for o, n in ranges]
        assert all(o >= 0 and n >= 0 and o + n <= self.nbytes for o, n in ranges)
        t = table(len(ranges))
        for i, (o, n) in enumerate(ranges):
            t[i]["src"], t[i]["n"], t[i]["stream_off"], t[i]["key"] = self.ptr + o, n, part_off + o, as_int32(key)
        return digest_table_device(t, None, workspace, self.device, stream)[1]

    def check(self, ranges, key, adlers, part_off=0, workspace=None, stream=None):
        """"Is this part the part I packed, and if not, which file first?": the ranges of `digests` against `adlers`, one Adler-32 per
        range (a host uint32 array, uploaded) -- one digest_table_device call and one digest check on the same stream, one synchronise,
        and the records never leave the device: 32 bytes come back, and n / 8 more only if a range is bad.  Returns (bad ranges, the
        lowest bad range or None, the bad ranges' indices as a uint64 array)."""
        ranges = [(int(o), int(n)) for o, n in ranges]
        assert all(o >= 0 and n >= 0 and o + n <= self.nbytes for o, n in ranges)
        adlers = np.ascontiguousarray(adlers, dtype=np.uint32)
        assert adlers.size == len(ranges)
        if not ranges:
            return _no_bad_entries()
        t = table(len(ranges))
        for i, (o, n) in enumerate(ranges):
            t[i]["src"], t[i]["n"], t[i]["stream_off"], t[i]["key"] = self.ptr + o, n, part_off + o, as_int32(key)
        return _table_call("modgpu_digest_table_device", t, TABLE_DTYPE, None, workspace, digest_table_workspace_bytes, self.device, stream,
                           "the device refused digest table entry {}; no record was written", fetch=_keep_on_device,
                           then=_check_behind(adlers, self.device))[1]

    def _extract_table(self, ranges, key, out, part_off):
        ranges = [(int(o), int(n)) for o, n in ranges]
        assert all(o >= 0 and n >= 0 and o + n <= self.nbytes for o, n in ranges)
        assert out is self or (out.device == self.device and sum(n for _, n in ranges) <= out.nbytes)
        t = table(len(ranges))
        at = 0
        for i, (o, n) in enumerate(ranges):
            t[i]["dst"], t[i]["src"] = (self.ptr + o if out is self else out.ptr + at), self.ptr + o
            t[i]["n"], t[i]["stream_off"], t[i]["key"] = n, part_off + o, as_int32(key)
            at += n
        return t

    def extract(self, ranges, key, out, part_off=0, side=DIGEST_OUTPUT, workspace=None, stream=None):
        """Cycles every range of `ranges` -- a list of (offset, n) -- of the part this buffer holds, each from stream offset part_off +
        offset, into `out` (another DeviceBuffer), packed end to end from offset 0, and returns one Adler-32 per range -- of what was
        stored, or with side=DIGEST_INPUT of what was read -- as a uint32 array: one cycle_digest_table_device call.  With `out is self`
        each range is cycled in place."""
        return cycle_digest_table_device(self._extract_table(ranges, key, out, part_off), None, side, workspace, self.device, stream)[1]

    def extract_checked(self, ranges, key, out, expect, part_off=0, side=DIGEST_OUTPUT, workspace=None, stream=None):
        """`extract`, and the call's records checked against `expect` -- one Adler-32 per range, a host uint32 array -- on the device,
        in the same stream: (the Adler-32 values as extract returns them, (bad ranges, the lowest bad range or None, the bad ranges'
        indices as a uint64 array))."""
        expect = np.ascontiguousarray(expect, dtype=np.uint32)
        t = self._extract_table(ranges, key, out, part_off)
        assert expect.size == t.size
        if not t.size:
            return _no_digest_results()[1], _no_bad_entries()
        (_, adlers), outcome = _table_call("modgpu_cycle_digest_table_device", t, TABLE_DTYPE, None, workspace, cycle_digest_table_workspace_bytes,
                                           self.device, stream, "the device refused cycle digest table entry {}; nothing was written", extra=(side,),
                                           fetch=digest_results, then=_check_behind(expect, self.device))
        return adlers, outcome

    def _convert_table(self, ranges, key_from, key_to, out, part_off):
        ranges = [(int(o), int(n)) for o, n in ranges]
        assert all(o >= 0 and n >= 0 and o + n <= self.nbytes for o, n in ranges)
        assert out is self or (out.device == self.device and all(o + n <= out.nbytes for o, n in ranges))
        t = rekey_table(len(ranges))
        for i, (o, n) in enumerate(ranges):
            t[i]["dst"], t[i]["src"], t[i]["n"] = out.ptr + o, self.ptr + o, n
            t[i]["off_from"] = t[i]["off_to"] = part_off + o
            t[i]["key_from"], t[i]["key_to"] = as_int32(key_from), as_int32(key_to)
        return t

    def convert(self, ranges, key_from, key_to, out, part_off=0, side=DIGEST_PLAIN, workspace=None, stream=None):
        """Converts every range of `ranges` -- a list of (offset, n) -- of the part this buffer holds from key_from to key_to, each at
        stream offset part_off + offset under both keys, into the same offset of `out` (another DeviceBuffer, or `self`: in place), and
        returns one Adler-32 per range -- of the plaintext between the two keystreams, or by `side` of what was stored or read -- as a
        uint32 array: one rekey_digest_table_device call."""
        return rekey_digest_table_device(self._convert_table(ranges, key_from, key_to, out, part_off), None, side, workspace, self.device, stream)[1]

    def convert_checked(self, ranges, key_from, key_to, out, expect, part_off=0, side=DIGEST_PLAIN, workspace=None, stream=None):
        """`convert`, and the call's records checked against `expect` -- one Adler-32 per range, a host uint32 array -- on the device,
        in the same stream: (the Adler-32 values as convert returns them, (bad ranges, the lowest bad range or None, the bad ranges'
        indices as a uint64 array))."""
        expect = np.ascontiguousarray(expect, dtype=np.uint32)
        t = self._convert_table(ranges, key_from, key_to, out, part_off)
        assert expect.size == t.size
        if not t.size:
            return _no_digest_results()[1], _no_bad_entries()
        (_, adlers), outcome = _table_call("modgpu_rekey_digest_table_device", t, REKEY_TABLE_DTYPE, None, workspace, rekey_digest_table_workspace_bytes,
                                           self.device, stream, "the device refused rekey digest table entry {}; nothing was written", extra=(side,),
                                           fetch=digest_results, then=_check_behind(expect, self.device))
        return adlers, outcome

    def move(self, dst_offset, src_offset, n, key_from=0, key_to=0, off_from=0, off_to=0, workspace=None, stream=None):
        """Moves n bytes inside the buffer from src_offset to dst_offset, the ranges overlapping in any way (memmove rules), rekeying
        on the way (rekey_move_device; with the default keys a plain memmove)."""
        assert max(dst_offset, src_offset) + n <= self.nbytes
        rekey_move_device(self.ptr + dst_offset, self.ptr + src_offset, n, key_from, key_to, off_from, off_to, workspace, self.device, stream)

    def compact(self, keep, key, part_off=0, workspace=None, stream=None):
        """Packs the surviving ranges `keep` -- a rising list of (offset, n) -- of the part this buffer holds end to end from the
        first range's offset, in one pass (compaction_table, rekey_move_table_device): each range slides down onto whatever lay
        before it and is rekeyed from its old stream offset part_off + offset to its new one.  Returns the new length: the offset
        just behind the last packed range."""
        keep = [(int(o), int(n)) for o, n in keep]
        assert all(o + n <= self.nbytes for o, n in keep)
        t = compaction_table(self.ptr, keep, key, part_off)
        rekey_move_table_device(t, None, workspace, self.device, stream)
        return keep[0][0] + sum(n for _, n in keep) if keep else 0

    def relayout(self, moves, key, key_to=None, part_off=0, workspace=None, stream=None):
        """Moves the segments `moves` -- a list of (src_off, dst_off, n), rising and disjoint on both sides, sliding either way -- of
        the part this buffer holds in one pass (relayout_table, rekey_relayout_table_device), each rekeyed from stream offset part_off
        + src_off under `key` to part_off + dst_off under key_to (None: `key`)."""
        moves = [(int(s), int(d), int(n)) for s, d, n in moves]
        assert all(min(s, d) >= 0 and max(s, d) + n <= self.nbytes for s, d, n in moves)
        rekey_relayout_table_device(relayout_table(self.ptr, moves, key, key_to, part_off), None, workspace, self.device, stream)

    def splice(self, edits, key, used, part_off=0, workspace=None, stream=None, *, key_to=None):
        """Splices the part this buffer holds in its first `used` bytes: for every (offset, old_len, new_len) of `edits` -- rising,
        disjoint -- old_len bytes at offset give way to a hole of new_len bytes, and every surviving segment slides by the sum of the
        size changes before it, up or down, in one pass under `key` -- or rekeyed to key_to on the way (splice_moves, relayout).  Returns
        (new_used, holes), `holes` the (new_offset, new_len) of every edit with new_len > 0; raises ValueError if new_used exceeds the
        buffer.  `fill` then fills all the holes in one call (after the splice's stream has been synchronised), under the key the part
        now has."""
        moves, new_used, holes = splice_moves(used, edits)
        if new_used > self.nbytes:
            raise ValueError(f"the spliced part needs {new_used} bytes, the buffer has {self.nbytes}")
        self.relayout(moves, key, key_to, part_off, workspace, stream)
        return new_used, holes

    def upload_ranges(self, items, key, part_off=0):
        """Uploads every (offset, array) of `items` into the part this buffer holds, each through the cipher from stream offset part_off
        + offset under `key`, in ONE list transfer (cycle_host_to_device_list); the ranges may not meet each other.  Synchronous, not
        ordered against the caller's streams."""
        items = [(int(o), a) for o, a in items]
        assert all(o >= 0 and o + _xfer_src(a)[1] <= self.nbytes for o, a in items)
        cycle_host_to_device_list([(self.ptr + o, a, key, part_off + o) for o, a in items], self.device)

    def download_ranges(self, ranges, key, outs, part_off=0):
        """Downloads every (offset, n) of `ranges` of the part this buffer holds into the array of `outs` at the same index (n bytes,
        writable), each through the cipher from stream offset part_off + offset under `key`, in ONE list transfer
        (cycle_device_to_host_list).  Returns `outs`."""
        ranges = [(int(o), int(n)) for o, n in ranges]
        assert len(outs) == len(ranges) and all(o >= 0 and o + n <= self.nbytes and _xfer_dst(a)[1] == n for (o, n), a in zip(ranges, outs))
        cycle_device_to_host_list([(self.ptr + o, a, key, part_off + o) for (o, _), a in zip(ranges, outs)], self.device)
        return outs

    def upload_ranges_digest(self, items, key, part_off=0, side=DIGEST_INPUT):
        """`upload_ranges`, and one Adler-32 per item taken in the same launch (cycle_host_to_device_list_digest) -- of the array as read
        (the plaintext, a packer's manifest), or with side=DIGEST_OUTPUT of what was stored -- returned as a uint32 array."""
        items = [(int(o), a) for o, a in items]
        assert all(o >= 0 and o + _xfer_src(a)[1] <= self.nbytes for o, a in items)
        return cycle_host_to_device_list_digest([(self.ptr + o, a, key, part_off + o) for o, a in items], side, None, self.device)[1]

    def download_ranges_checked(self, ranges, key, outs, expect, part_off=0, side=DIGEST_OUTPUT):
        """`download_ranges`, one Adler-32 per range taken in the same launch (cycle_device_to_host_list_digest) -- of what was stored
        in `outs`, or with side=DIGEST_INPUT of the device bytes as read -- and the call's records checked against `expect`, one Adler-32
        per range (a host uint32 array), on the device where they lie (digest_check_device): (the Adler-32 values as a uint32 array,
        (bad ranges, the lowest bad range or None, the bad ranges' indices as a uint64 array))."""
        ranges = [(int(o), int(n)) for o, n in ranges]
        expect = np.ascontiguousarray(expect, dtype=np.uint32)
        assert len(outs) == len(ranges) == expect.size and all(o >= 0 and o + n <= self.nbytes and _xfer_dst(a)[1] == n for (o, n), a in zip(ranges, outs))
        if not ranges:
            return _no_digest_results()[1], _no_bad_entries()
        records = DeviceBuffer(DIGEST_RESULT_DTYPE.itemsize * len(ranges), self.device)
        try:
            _, adlers = cycle_device_to_host_list_digest([(self.ptr + o, a, key, part_off + o) for (o, _), a in zip(ranges, outs)], side, records, self.device)
            return adlers, digest_check_device(records, expect, len(ranges), device=self.device)
        finally:
            records.free()

    def fill(self, holes, bufs, key, part_off=0):
        """Fills the `holes` that `splice` returned -- (new_offset, new_len) each -- with the plaintext arrays `bufs`, one per hole and
        new_len bytes long, under the key the part now has: ONE list transfer for all of them (upload_ranges).  Not ordered against the
        caller's streams: synchronise the splice's stream first."""
        holes = [(int(o), int(n)) for o, n in holes]
        assert len(bufs) == len(holes) and all(_xfer_src(b)[1] == n for (_, n), b in zip(holes, bufs))
        self.upload_ranges([(o, b) for (o, _), b in zip(holes, bufs)], key, part_off)

    def sync(self, stream=None):
        _check(self._lib.modgpu_sync(self.device, _vp(stream or 0)))

    def free(self):
        if self.ptr:
            _check(self._lib.modgpu_free(_vp(self.ptr), self.device))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

"""vigor_amd — MI355X-native Vigor per-packet path (host-side mirror).

Thin ctypes layer over libvigpath.so (include/vigpath.h), the C-ABI the HIP
kernels sit behind. There is no CPU fallback: if the library or a GPU is
missing, every entry point raises. The CPU restatement used to check results
lives in oracle/ and is test infrastructure only.
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
# VIGPATH_LIB: another build of the same ABI, for diagnostics (A/B builds)
LIB_PATH = os.environ.get("VIGPATH_LIB") or os.path.join(PKG, "libvigpath.so")
MAX_DEV = 32
FLOOD_FRAME = 0xFFFF

VP_OK, VP_EINVAL, VP_ENOMEM, VP_EIO, VP_ENOTSUP = 0, -22, -12, -5, -95
VP_ESTATE = -71
_ERR = {VP_EINVAL: "EINVAL", VP_ENOMEM: "ENOMEM", VP_EIO: "EIO (HIP)",
        VP_ESTATE: "ESTATE (device protocol)",
        VP_ENOTSUP: "ENOTSUP"}


class VigpathError(RuntimeError):
    def __init__(self, rc: int, what: str, detail: str = ""):
        super().__init__(f"{what}: {_ERR.get(rc, rc)}" + (f" [{detail}]" if detail else ""))
        self.rc = rc
        self.detail = detail


class TableStatsC(C.Structure):
    """vp_table_stats (include/vigpath.h)."""
    _fields_ = [("live", C.c_uint64), ("shard_live", C.c_uint64),
                ("tombstones", C.c_uint64), ("buckets", C.c_uint64),
                ("rebuilds", C.c_uint64), ("layout", C.c_uint32),
                ("pad", C.c_uint32)]


class StateMarkC(C.Structure):
    """vp_state_mark_t (include/vigpath.h)."""
    _fields_ = [("seq", C.c_uint64), ("epoch", C.c_uint64)]


STATE_DELTA_MAGIC = 0x44535056  # VP_STATE_DELTA_MAGIC, the bytes "VPSD"
STATE_DELTA_VERSION = 1         # VP_STATE_DELTA_VERSION


class VpLookupOutC(C.Structure):
    """vp_lookup_out (include/vigpath.h): device pointers, any may be NULL."""
    _fields_ = [("index", C.c_void_p), ("ts", C.c_void_p), ("key", C.c_void_p),
                ("value", C.c_void_p)]


LOOKUP_MISS = 0xFFFFFFFF  # VP_LOOKUP_MISS


class ServeStatsC(C.Structure):
    """vp_serve_stats (include/vigpath.h)."""
    _fields_ = [("packets_one", C.c_uint64), ("bursts", C.c_uint64),
                ("burst_packets", C.c_uint64), ("declined", C.c_uint64),
                ("launches", C.c_uint64)]


class ServeExpiryStatsC(C.Structure):
    """vp_serve_expiry_stats (include/vigpath.h)."""
    _fields_ = [("seeds", C.c_uint64), ("expired", C.c_uint64),
                ("walks", C.c_uint64), ("handed", C.c_uint64),
                ("splits", C.c_uint64)]


class TxStatsC(C.Structure):
    """vp_tx_stats (include/vigpath.h)."""
    _fields_ = [("packets", C.c_uint64 * MAX_DEV), ("bytes", C.c_uint64 * MAX_DEV),
                ("dropped", C.c_uint64), ("flooded", C.c_uint64),
                ("bad_port", C.c_uint64)]


class TxListsC(C.Structure):
    """vp_tx_lists (include/vigpath.h): device pointers."""
    _fields_ = [("idx", C.c_void_p), ("cap", C.c_uint32), ("offset", C.c_void_p),
                ("stats", C.c_void_p)]


class TxFramesC(C.Structure):
    """vp_tx_frames (include/vigpath.h): device pointers."""
    _fields_ = [("data", C.c_void_p), ("cap_bytes", C.c_uint64), ("port_off", C.c_void_p),
                ("pos", C.c_void_p)]


class TxNextC(C.Structure):
    """vp_tx_next (include/vigpath.h): device pointers."""
    _fields_ = [("frames", C.c_void_p), ("slot", C.c_uint32), ("cap", C.c_uint32),
                ("len", C.c_void_p), ("now", C.c_void_p), ("src", C.c_void_p),
                ("count", C.c_void_p)]


class RxStreamC(C.Structure):
    """vp_rx_stream (include/vigpath.h): device pointers."""
    _fields_ = [("data", C.c_void_p), ("bytes", C.c_uint64), ("n", C.c_uint32),
                ("pos", C.c_void_p), ("sel", C.c_void_p), ("meta_n", C.c_uint32),
                ("len", C.c_void_p), ("now", C.c_void_p), ("now0", C.c_int64),
                ("now_step", C.c_int64)]


TX_MERGE_MAX = 8  # VP_TX_MERGE_MAX
RX_MERGE_MAX = 8  # VP_RX_MERGE_MAX


class RxQueueC(C.Structure):
    """vp_rx_queue (include/vigpath.h): one stream of a vp_rx_merge call."""
    _fields_ = [("stream", RxStreamC), ("in_port", C.c_uint32)]

RET_SKIP, RET_DROP = 0x10000, 0x10001  # VP_RET_SKIP, VP_RET_DROP


class TxReturnStatsC(C.Structure):
    """vp_tx_return_stats (include/vigpath.h)."""
    _fields_ = [("returned", C.c_uint64), ("dropped", C.c_uint64), ("skipped", C.c_uint64),
                ("dup", C.c_uint64), ("bad_home", C.c_uint64)]


class TxWayHomeC(C.Structure):
    """vp_tx_way_home (include/vigpath.h): home and stats are device pointers."""
    _fields_ = [("home", C.c_void_p), ("port", C.c_uint32 * MAX_DEV),
                ("on_drop", C.c_uint32), ("on_flood", C.c_uint32), ("on_bad", C.c_uint32),
                ("stats", C.c_void_p)]


class TxSourceC(C.Structure):
    """vp_tx_source (include/vigpath.h): one list of a vp_tx_merge call."""
    _fields_ = [("ctx", C.c_void_p), ("batch", C.c_void_p), ("lists", C.c_void_p),
                ("port", C.c_uint32), ("in_port", C.c_uint32), ("key", C.c_void_p)]


class TxMergedC(C.Structure):
    """vp_tx_merged (include/vigpath.h): device pointers."""
    _fields_ = [("frames", C.c_void_p), ("slot", C.c_uint32), ("cap", C.c_uint32),
                ("len", C.c_void_p), ("now", C.c_void_p), ("in_dev", C.c_void_p),
                ("key", C.c_void_p), ("src", C.c_void_p), ("which", C.c_void_p),
                ("count", C.c_void_p)]


CHAIN_MAX_STAGES = 16  # VP_CHAIN_MAX_STAGES
CABLE_SLOTS, CABLE_STREAM = 0, 1  # VP_CABLE_SLOTS, VP_CABLE_STREAM


class ChainLinkC(C.Structure):
    """vp_chain_link (include/vigpath.h)."""
    _fields_ = [("from", C.c_uint32), ("out_port", C.c_uint32), ("to", C.c_uint32),
                ("in_port", C.c_uint32)]


class ChainExitC(C.Structure):
    """vp_chain_exit (include/vigpath.h)."""
    _fields_ = [("stage", C.c_uint32), ("port", C.c_uint32), ("ext_port", C.c_uint32)]


class ChainConfigC(C.Structure):
    """vp_chain_config (include/vigpath.h): host pointers."""
    _fields_ = [("stages", C.POINTER(C.c_void_p)), ("n_stages", C.c_uint32),
                ("links", C.POINTER(ChainLinkC)), ("n_links", C.c_uint32),
                ("exits", C.POINTER(ChainExitC)), ("n_exits", C.c_uint32),
                ("cable", C.c_uint32)]


class ChainViewC(C.Structure):
    """vp_chain_view (include/vigpath.h): device pointers."""
    _fields_ = [("n", C.c_uint32), ("slot", C.c_uint32), ("frames", C.c_void_p),
                ("len", C.c_void_p), ("out_dev", C.c_void_p), ("in_dev", C.c_void_p),
                ("in_port", C.c_uint32), ("now", C.c_void_p), ("origin", C.c_void_p)]


# packets per block of vp_tx_build's kernels (vp_tx.hip kTxBlockPackets)
TX_BLOCK_PACKETS = 2048

MacTable = (C.c_uint8 * 6) * MAX_DEV


class NatConfigC(C.Structure):
    """vp_nat_config (vignat/nat_config.h:5-31)."""
    _fields_ = [("wan_device", C.c_uint16), ("lan_main_device", C.c_uint16),
                ("start_port", C.c_uint16), ("external_addr", C.c_uint32),
                ("expiration_time", C.c_uint32), ("max_flows", C.c_uint32),
                ("n_devices", C.c_uint16), ("device_macs", MacTable),
                ("endpoint_macs", MacTable)]


class BridgeRuleC(C.Structure):
    _fields_ = [("mac", C.c_uint8 * 6), ("device_from", C.c_int32),
                ("device_to", C.c_int32)]


class BridgeConfigC(C.Structure):
    """vp_bridge_config (vigbridge/bridge_config.h:8-18)."""
    _fields_ = [("expiration_time", C.c_uint32), ("dyn_capacity", C.c_uint32),
                ("n_devices", C.c_uint16), ("n_static", C.c_uint32),
                ("static_rules", C.POINTER(BridgeRuleC))]


class LbConfigC(C.Structure):
    """vp_lb_config (viglb/lb_config.h:8-38)."""
    _fields_ = [("flow_capacity", C.c_uint32),
                ("flow_expiration_time", C.c_uint32),
                ("backend_capacity", C.c_uint32), ("cht_height", C.c_uint32),
                ("backend_expiration_time", C.c_uint32),
                ("wan_device", C.c_uint16), ("n_devices", C.c_uint16),
                ("device_macs", MacTable)]


class FwConfigC(C.Structure):
    """vp_fw_config (vigfw/fw_config.h:9-24)."""
    _fields_ = [("wan_device", C.c_uint16), ("expiration_time", C.c_uint32),
                ("max_flows", C.c_uint32), ("n_devices", C.c_uint16),
                ("device_macs", MacTable), ("endpoint_macs", MacTable)]


class PolConfigC(C.Structure):
    """vp_pol_config (vigpol/policer_config.h:8-24)."""
    _fields_ = [("lan_device", C.c_uint16), ("wan_device", C.c_uint16),
                ("rate", C.c_uint64), ("burst", C.c_uint64),
                ("dyn_capacity", C.c_uint32), ("n_devices", C.c_uint16)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_size_t)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p,
                           C.POINTER(C.c_size_t), C.c_void_p,
                           C.POINTER(C.c_size_t))

SHARD_REPLICATED, SHARD_OWNER = 0, 1  # vp_shard_mode


class CommOpsC(C.Structure):
    """vp_comm_ops: host-memory collectives supplied by the caller."""
    _fields_ = [("user", C.c_void_p), ("allgather", ALLGATHER_FN),
                ("allreduce_max_u64", ALLREDUCE_FN),
                ("alltoallv", ALLTOALLV_FN)]


class DevBatchC(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("slot", C.c_uint32), ("n", C.c_uint32),
                ("len", C.c_void_p), ("in_dev", C.c_void_p),
                ("now", C.c_void_p), ("now0", C.c_int64),
                ("now_step", C.c_int64), ("out_dev", C.c_void_p), ("in_port", C.c_uint32)]


class MbufBatchC(C.Structure):
    """vp_mbuf_batch (include/vigpath.h): a DPDK-shaped host batch."""
    _fields_ = [("n", C.c_uint32), ("frames", C.c_void_p), ("len", C.c_void_p),
                ("in_dev", C.c_void_p), ("now", C.c_void_p), ("now0", C.c_int64),
                ("now_step", C.c_int64), ("out_dev", C.c_void_p)]


# every symbol include/vigpath.h declares
EXPORTS = ["vp_nat_create", "vp_bridge_create", "vp_lb_create", "vp_fw_create",
           "vp_pol_create", "vp_pol_dump", "vp_destroy", "vp_process_device", "vp_process_batch",
           "vp_process_host", "vp_process_host_batch", "vp_nat_dump", "vp_bridge_dump", "vp_lb_dump",
           "vp_fw_dump", "vp_comm_unique_id", "vp_attach_rccl",
           "vp_attach_comm", "vp_shard_mode", "vp_sync_state", "vp_live_count",
           "vp_kernel_timing", "vp_last_kernel_ms", "vp_version", "vp_table_stats_get",
           "vp_last_error", "vp_register_host", "vp_unregister_host", "vp_process_mbufs",
           "vp_last_stage_ms", "vp_stage_ms", "vp_comm_abort", "vp_probe_slots",
           "vp_probe_slots_w", "vp_probe_slots_p", "vp_process_one", "vp_last_kernel", "vp_serve_stats_get",
           "vp_serve_expiry_stats_get", "vp_tx_build", "vp_tx_pack", "vp_tx_rebatch",
           "vp_tx_merge", "vp_rx_unpack", "vp_rx_merge", "vp_tx_return", "vp_chain_create", "vp_chain_destroy",
           "vp_chain_run", "vp_chain_view_get", "vp_chain_process_device",
           "vp_state_size", "vp_state_save", "vp_state_load", "vp_state_mark",
           "vp_state_delta_size", "vp_state_delta_save", "vp_state_follow",
           "vp_state_delta_apply", "vp_table_lookup", "vp_table_entries",
           "vp_table_value_size", "vp_table_erase", "vp_table_free"]

_libs = {}


def lib(path: str | None = None):
    """Load libvigpath.so (or, for diagnostics, another build of the same
    ABI); raises if it has not been built."""
    path = path or LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(f"{path} missing: run __graft_entry__.build()")
    L = C.CDLL(path)
    L.vp_version.restype = C.c_char_p
    for name in ("vp_nat_create", "vp_bridge_create", "vp_lb_create",
                 "vp_fw_create"):
        getattr(L, name).restype = C.c_int
    L.vp_fw_create.argtypes = [C.POINTER(FwConfigC), C.c_int,
                               C.POINTER(C.c_void_p)]
    L.vp_fw_dump.argtypes = [C.c_void_p] * 5
    L.vp_fw_dump.restype = C.c_int
    L.vp_pol_create.restype = C.c_int
    L.vp_pol_create.argtypes = [C.POINTER(PolConfigC), C.c_int,
                                C.POINTER(C.c_void_p)]
    L.vp_pol_dump.argtypes = [C.c_void_p] * 6
    L.vp_pol_dump.restype = C.c_int
    L.vp_nat_create.argtypes = [C.POINTER(NatConfigC), C.c_int,
                                C.POINTER(C.c_void_p)]
    L.vp_bridge_create.argtypes = [C.POINTER(BridgeConfigC), C.c_int,
                                   C.POINTER(C.c_void_p)]
    L.vp_lb_create.argtypes = [C.POINTER(LbConfigC), C.c_int,
                               C.POINTER(C.c_void_p)]
    L.vp_destroy.argtypes = [C.c_void_p]
    L.vp_destroy.restype = None
    L.vp_process_device.argtypes = [C.c_void_p, C.POINTER(DevBatchC),
                                    C.c_void_p]
    L.vp_process_device.restype = C.c_int
    L.vp_process_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p,
                                  C.c_void_p, C.c_uint32, C.c_void_p,
                                  C.c_void_p, C.c_void_p]
    L.vp_process_host.restype = C.c_int
    L.vp_process_host_batch.argtypes = [C.c_void_p, C.POINTER(DevBatchC)]
    L.vp_process_host_batch.restype = C.c_int
    L.vp_process_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p,
                                   C.POINTER(C.c_void_p), C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    L.vp_process_batch.restype = C.c_int
    L.vp_process_one.argtypes = [C.c_void_p, C.c_uint16, C.c_void_p, C.c_uint16,
                                 C.c_int64, C.POINTER(C.c_uint16)]
    L.vp_process_one.restype = C.c_int
    L.vp_process_mbufs.argtypes = [C.c_void_p, C.POINTER(MbufBatchC)]
    L.vp_process_mbufs.restype = C.c_int
    L.vp_register_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.vp_register_host.restype = C.c_int
    L.vp_unregister_host.argtypes = [C.c_void_p, C.c_void_p]
    L.vp_unregister_host.restype = C.c_int
    L.vp_nat_dump.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.vp_nat_dump.restype = C.c_int
    L.vp_bridge_dump.argtypes = [C.c_void_p] * 5
    L.vp_bridge_dump.restype = C.c_int
    L.vp_lb_dump.argtypes = [C.c_void_p] * 10
    L.vp_lb_dump.restype = C.c_int
    L.vp_comm_unique_id.argtypes = [C.c_void_p]
    L.vp_comm_unique_id.restype = C.c_int
    L.vp_attach_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.vp_attach_rccl.restype = C.c_int
    L.vp_attach_comm.argtypes = [C.c_void_p, C.POINTER(CommOpsC), C.c_int,
                                 C.c_int]
    L.vp_attach_comm.restype = C.c_int
    L.vp_shard_mode.argtypes = [C.c_void_p, C.c_int]
    L.vp_shard_mode.restype = C.c_int
    L.vp_sync_state.argtypes = [C.c_void_p]
    L.vp_sync_state.restype = C.c_int
    L.vp_comm_abort.argtypes = [C.c_void_p]
    L.vp_comm_abort.restype = C.c_int
    L.vp_probe_slots.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                 C.POINTER(C.c_float)]
    L.vp_probe_slots.restype = C.c_int
    L.vp_probe_slots_w.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                   C.POINTER(C.c_float)]
    L.vp_probe_slots_w.restype = C.c_int
    L.vp_probe_slots_p.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.vp_probe_slots_p.restype = C.c_int
    L.vp_live_count.argtypes = [C.c_void_p]
    L.vp_live_count.restype = C.c_int64
    L.vp_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float),
                                    C.POINTER(C.c_int)]
    L.vp_last_kernel_ms.restype = C.c_int
    L.vp_last_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]
    L.vp_last_stage_ms.restype = C.c_int
    L.vp_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int, C.POINTER(C.c_int)]
    L.vp_stage_ms.restype = C.c_int
    L.vp_last_kernel.argtypes = [C.c_void_p]
    L.vp_last_kernel.restype = C.c_char_p
    L.vp_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    L.vp_kernel_timing.restype = C.c_int
    L.vp_table_stats_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(TableStatsC)]
    L.vp_table_stats_get.restype = C.c_int
    L.vp_serve_stats_get.argtypes = [C.c_void_p, C.POINTER(ServeStatsC)]
    L.vp_serve_stats_get.restype = C.c_int
    L.vp_serve_expiry_stats_get.argtypes = [C.c_void_p, C.POINTER(ServeExpiryStatsC)]
    L.vp_serve_expiry_stats_get.restype = C.c_int
    L.vp_tx_build.argtypes = [C.c_void_p, C.POINTER(DevBatchC), C.POINTER(TxListsC),
                              C.c_void_p]
    L.vp_tx_build.restype = C.c_int
    L.vp_tx_pack.argtypes = [C.c_void_p, C.POINTER(DevBatchC), C.POINTER(TxListsC),
                             C.POINTER(TxFramesC), C.c_void_p]
    L.vp_tx_pack.restype = C.c_int
    L.vp_tx_rebatch.argtypes = [C.c_void_p, C.POINTER(DevBatchC), C.POINTER(TxListsC),
                                C.c_uint32, C.POINTER(TxNextC), C.c_void_p]
    L.vp_tx_rebatch.restype = C.c_int
    L.vp_tx_merge.argtypes = [C.c_void_p, C.POINTER(TxSourceC), C.c_uint32,
                              C.POINTER(TxMergedC), C.c_void_p]
    L.vp_tx_merge.restype = C.c_int
    L.vp_rx_unpack.argtypes = [C.c_void_p, C.POINTER(RxStreamC), C.POINTER(TxNextC),
                               C.c_void_p]
    L.vp_rx_unpack.restype = C.c_int
    L.vp_rx_merge.argtypes = [C.c_void_p, C.POINTER(RxQueueC), C.c_uint32,
                              C.POINTER(TxMergedC), C.c_void_p]
    L.vp_rx_merge.restype = C.c_int
    L.vp_tx_return.argtypes = [C.c_void_p, C.POINTER(DevBatchC), C.POINTER(DevBatchC),
                               C.POINTER(TxWayHomeC), C.c_void_p]
    L.vp_tx_return.restype = C.c_int
    L.vp_chain_create.argtypes = [C.POINTER(ChainConfigC), C.POINTER(C.c_void_p)]
    L.vp_chain_create.restype = C.c_int
    L.vp_chain_destroy.argtypes = [C.c_void_p]
    L.vp_chain_destroy.restype = None
    L.vp_chain_run.argtypes = [C.c_void_p, C.POINTER(DevBatchC), C.c_void_p]
    L.vp_chain_run.restype = C.c_int
    L.vp_chain_view_get.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(ChainViewC)]
    L.vp_chain_view_get.restype = C.c_int
    L.vp_chain_process_device.argtypes = [C.c_void_p, C.POINTER(DevBatchC),
                                          C.POINTER(TxReturnStatsC), C.c_void_p]
    L.vp_chain_process_device.restype = C.c_int
    L.vp_state_size.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.vp_state_size.restype = C.c_int
    L.vp_state_save.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.vp_state_save.restype = C.c_int
    L.vp_state_load.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.vp_state_load.restype = C.c_int
    MP = C.POINTER(StateMarkC)
    L.vp_state_mark.argtypes = [C.c_void_p, MP]
    L.vp_state_mark.restype = C.c_int
    L.vp_state_delta_size.argtypes = [C.c_void_p, MP, C.POINTER(C.c_uint64)]
    L.vp_state_delta_size.restype = C.c_int
    L.vp_state_delta_save.argtypes = [C.c_void_p, MP, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), MP]
    L.vp_state_delta_save.restype = C.c_int
    L.vp_state_follow.argtypes = [C.c_void_p, MP]
    L.vp_state_follow.restype = C.c_int
    L.vp_state_delta_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.vp_state_delta_apply.restype = C.c_int
    for name in ("vp_table_lookup", "vp_table_entries"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p,
                                     C.POINTER(VpLookupOutC), C.c_void_p]
        getattr(L, name).restype = C.c_int
    L.vp_table_value_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
    L.vp_table_value_size.restype = C.c_int
    for name in ("vp_table_erase", "vp_table_free"):
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p,
                                     C.POINTER(VpLookupOutC), C.POINTER(C.c_uint32), C.c_void_p]
        getattr(L, name).restype = C.c_int
    L.vp_last_error.argtypes = []
    L.vp_last_error.restype = C.c_char_p
    _libs[path] = L
    return L


_DETAILED = (-5, -12, -71)  # VP_EIO, VP_ENOMEM, VP_ESTATE record vp_last_error()


def _check(rc: int, what: str, L=None):
    """Raise VigpathError for a failing vp_* return code. `L` is the library
    that made the call (the first one loaded if omitted). Only the codes that
    record a reason (VP_EIO / VP_ENOMEM / VP_ESTATE) carry vp_last_error():
    the others record nothing, and the thread's text would belong to an
    earlier failure."""
    if rc != 0:
        detail = ""
        if L is None:
            L = next(iter(_libs.values()), None)
        if L is not None and rc in _DETAILED:
            detail = (L.vp_last_error() or b"").decode(errors="replace")
        raise VigpathError(rc, what, detail)


from .nf import Bridge, Fw, Lb, Nat, NfBase, Pol  # noqa: E402,F401
from .chain import Chain  # noqa: E402,F401
from .cchain import CChain  # noqa: E402,F401
from .config import (bridge_config_from_args, fw_config_from_args,  # noqa
                     lb_config_from_args, nat_config_from_args,
                     pol_config_from_args)

"""Loader for libldpc_hip.so (the C ABI of include/ldpc_hip.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C
myldpccppapi_amd/csrc`.  There is no fallback: if it is missing, loading fails
loudly, and every compute entry point fails without a HIP device.
"""
import ctypes
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# LDPC_HIP_LIB: load another build of the same library (kernel-variant experiments); read by this
# Python loader only -- the library itself reads no environment variables
LIB_PATH = os.environ.get("LDPC_HIP_LIB") or os.path.join(_HERE, "libldpc_hip.so")
_lib = None


class LdpcError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("ldpc_hip error %d: %s" % (code, message))
        self.code = code


class DecoderConfig(ctypes.Structure):
    """Mirror of `ldpc_decoder_config` (include/ldpc_hip.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("K", ctypes.c_int32),
                ("max_batch", ctypes.c_int32), ("algo", ctypes.c_int32),
                ("msg_dtype", ctypes.c_int32), ("max_iter", ctypes.c_int32),
                ("llr_scale", ctypes.c_float), ("early_term", ctypes.c_int32),
                ("device", ctypes.c_int32), ("layer_rows", ctypes.c_int32),
                ("pack_mode", ctypes.c_int32), ("frames_per_lane", ctypes.c_int32),
                ("poll_interval", ctypes.c_int32),
                ("tune_flags", ctypes.c_int32), ("tune_rows_per_wave", ctypes.c_int32),
                ("tune_cols_per_wave", ctypes.c_int32), ("tune_link_rows", ctypes.c_int32),
                ("tune_compact", ctypes.c_int32), ("tune_ldsp_grid", ctypes.c_int32),
                ("tune_ldsp_shape", ctypes.c_int32), ("tune_place", ctypes.c_int32),
                ("host_input", ctypes.c_int32),
                ("host_copy_threads", ctypes.c_int32), ("tune_q_order", ctypes.c_int32),
                ("ms_scale", ctypes.c_float), ("ms_offset", ctypes.c_float)]


class DecoderConfigCrc(DecoderConfig):
    """The whole of `ldpc_decoder_config`: DecoderConfig is the struct as it was before crc_kind / crc_bits (a size the
    library still accepts, CRC off, and the one ldpc_decoder_config_init fills); this one has the two fields behind it and
    is initialised with ldpc_decoder_config_init_sized(cfg, sizeof)."""
    _fields_ = [("crc_kind", ctypes.c_int32), ("crc_bits", ctypes.c_int32)]


class _MsgTailNames(ctypes.Structure):
    """The names the header gives the second and third of the three ints (the first is post_bits)."""
    _fields_ = [("_post_bits", ctypes.c_int32), ("bp_frac_bits", ctypes.c_int32), ("msg_reserved3", ctypes.c_int32)]


class _MsgTail(ctypes.Union):
    """The three ints behind msg_bits: `post_bits; bp_frac_bits; msg_reserved3` in the header, which were `msg_reserved[3]`."""
    _anonymous_ = ("_names",)
    _fields_ = [("msg_reserved", ctypes.c_int32 * 3), ("post_bits", ctypes.c_int32), ("_names", _MsgTailNames)]


class DecoderConfigMsg(DecoderConfigCrc):
    """The whole of `ldpc_decoder_config`: DecoderConfigCrc is the struct as it was before msg_bits (a size the library
    still accepts, msg_bits = 0); this one has msg_bits and the three ints behind it.  The first of them is post_bits
    (LDPC_ALGO_LAYERED_FX and LAYERED_BP_FX), which aliases msg_reserved[0]; the second is bp_frac_bits (LDPC_ALGO_LAYERED_BP_FX),
    which aliases msg_reserved[1]; the third is reserved and must be 0."""
    _anonymous_ = ("_tail",)
    _fields_ = [("msg_bits", ctypes.c_int32), ("_tail", _MsgTail)]


class DecoderConfigBf(DecoderConfigMsg):
    """The whole of `ldpc_decoder_config`: DecoderConfigMsg is the struct as it was before bf_threshold (a size the library
    still accepts, all thresholds 0); this one has the sixteen round offsets of LDPC_ALGO_BITFLIP behind it."""
    _fields_ = [("bf_threshold", ctypes.c_int32 * 16)]


class DecodeStats(ctypes.Structure):
    """Mirror of `ldpc_decode_stats`."""
    _fields_ = [("iterations_launched", ctypes.c_int32), ("batch_time", ctypes.c_int32),
                ("frames", ctypes.c_int64), ("frames_converged", ctypes.c_int64),
                ("ms_total", ctypes.c_float), ("ms_check", ctypes.c_float),
                ("ms_var", ctypes.c_float), ("ms_other", ctypes.c_float),
                ("launches_check", ctypes.c_int32), ("launches_var", ctypes.c_int32),
                ("frame_rounds", ctypes.c_int64)]


class KernelTime(ctypes.Structure):
    """Mirror of `ldpc_kernel_time`."""
    _fields_ = [("phase", ctypes.c_int32), ("degree", ctypes.c_int32), ("launches", ctypes.c_int32),
                ("ms_total", ctypes.c_float), ("bytes_total", ctypes.c_int64), ("name", ctypes.c_char * 64),
                ("bytes_moved", ctypes.c_int64)]


class RateSpec(ctypes.Structure):
    """Mirror of `ldpc_rate_spec`."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("N", ctypes.c_int32), ("punctured", ctypes.c_int32),
                ("filler_lo", ctypes.c_int32), ("filler_hi", ctypes.c_int32),
                ("fill_llr", ctypes.c_float), ("erasure_llr", ctypes.c_float)]


class ModemSpec(ctypes.Structure):
    """Mirror of `ldpc_modem_spec`."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("Qm", ctypes.c_int32), ("interleave", ctypes.c_int32)]


class TbSpec(ctypes.Structure):
    """Mirror of `ldpc_tb_spec`."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("A", ctypes.c_int32), ("tb_crc", ctypes.c_int32), ("C", ctypes.c_int32),
                ("cb_crc", ctypes.c_int32), ("K", ctypes.c_int32)]


class BchSpec(ctypes.Structure):
    """Mirror of `ldpc_bch_spec`."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("m", ctypes.c_int32), ("prim", ctypes.c_uint32), ("t", ctypes.c_int32),
                ("n", ctypes.c_int32), ("row_bytes", ctypes.c_int32)]


#: every symbol include/ldpc_hip.h declares
EXPORTS = (
    "ldpc_abi_version", "ldpc_last_error", "ldpc_device_count", "ldpc_graph_create",
    "ldpc_graph_destroy", "ldpc_graph_info", "ldpc_decoder_config_init", "ldpc_decoder_create",
    "ldpc_decoder_create_multi", "ldpc_shard_range", "ldpc_decoder_destroy", "ldpc_decode", "ldpc_decode_device", "ldpc_out_bytes",
    "ldpc_decoder_set_timing", "ldpc_decoder_stats", "ldpc_decoder_kernel_times", "ldpc_decoder_set_tap",
    "ldpc_decoder_dump", "ldpc_awgn_device", "ldpc_count_errors_device", "ldpc_hbm_probe_device", "ldpc_hbm_sustained_device",
    "ldpc_host_block_plan", "ldpc_host_locked_ranges", "ldpc_decoder_link_form", "ldpc_decoder_placement", "ldpc_decoder_array_addresses",
    "ldpc_parity_structure", "ldpc_encoder_create", "ldpc_encoder_destroy", "ldpc_encode_device", "ldpc_encode", "ldpc_code_bytes",
    "ldpc_rate_spec_init", "ldpc_rate_lengths", "ldpc_rate_index", "ldpc_rate_match_device", "ldpc_rate_recover_device",
    "ldpc_rate_match", "ldpc_rate_recover",
    "ldpc_modem_spec_init", "ldpc_modem_symbol_floats", "ldpc_modem_index", "ldpc_modem_points", "ldpc_modem_transmit_device",
    "ldpc_modem_demap_device", "ldpc_modem_transmit", "ldpc_modem_demap",
    "ldpc_tb_spec_init", "ldpc_tb_layout", "ldpc_crc_bits", "ldpc_tb_attach_device", "ldpc_tb_check_device", "ldpc_tb_tally_device",
    "ldpc_tb_attach", "ldpc_tb_check",
    "ldpc_decoder_crc_stops", "ldpc_crc_weights", "ldpc_tb_frame_crc", "ldpc_decoder_config_init_sized",
    "ldpc_decode_soft_device", "ldpc_decode_soft",
    "ldpc_decode_typed_device", "ldpc_decode_soft_typed_device", "ldpc_decode_typed", "ldpc_decode_soft_typed",
    "ldpc_llr_quantize_device",
    "ldpc_bch_spec_init", "ldpc_bch_layout", "ldpc_bch_generator", "ldpc_bch_encode_device", "ldpc_bch_decode_device",
    "ldpc_bch_tally_device", "ldpc_bch_encode", "ldpc_bch_decode",
    "ldpc_osd_create", "ldpc_osd_destroy", "ldpc_osd_device", "ldpc_osd_run", "ldpc_osd_info",
    "ldpc_graph_systematic_order", "ldpc_parity_dense", "ldpc_parity_dense_rows", "ldpc_encoder_create_dense",
    "ldpc_bp_fx_table",
)


def load():
    """dlopen the library and declare the prototypes.  Raises OSError if the
    library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C myldpccppapi_amd/csrc`" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same
    # soname).  If torch is importable, let it load first so both share it.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    i32p = ctypes.POINTER(ctypes.c_int32)
    i64p = ctypes.POINTER(ctypes.c_int64)
    vp = ctypes.c_void_p
    L.ldpc_abi_version.restype = ctypes.c_int
    L.ldpc_last_error.restype = ctypes.c_char_p
    L.ldpc_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
    L.ldpc_graph_create.argtypes = [i32p, i32p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32,
                                    ctypes.POINTER(vp)]
    L.ldpc_graph_destroy.argtypes = [vp]
    L.ldpc_graph_info.argtypes = [vp, i32p, i32p, i64p, i32p, i32p]
    L.ldpc_decoder_config_init.argtypes = [ctypes.POINTER(DecoderConfig)]
    L.ldpc_decoder_config_init.restype = None
    L.ldpc_decoder_config_init_sized.argtypes = [ctypes.POINTER(DecoderConfig), ctypes.c_uint32]
    L.ldpc_decoder_create.argtypes = [vp, ctypes.POINTER(DecoderConfig), ctypes.POINTER(vp)]
    L.ldpc_decoder_create_multi.argtypes = [vp, ctypes.POINTER(DecoderConfig), i32p, ctypes.c_int32,
                                            ctypes.POINTER(vp)]
    L.ldpc_shard_range.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i64p, i64p]
    L.ldpc_decoder_destroy.argtypes = [vp]
    L.ldpc_decode.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp]
    L.ldpc_decode_device.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp]
    L.ldpc_decode_soft.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, ctypes.c_int32]
    L.ldpc_decode_soft_device.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, ctypes.c_int32, vp]
    f32, i32 = ctypes.c_float, ctypes.c_int32
    L.ldpc_decode_typed.argtypes = [vp, vp, i32, f32, ctypes.c_int64, vp, ctypes.c_int64, vp]
    L.ldpc_decode_typed_device.argtypes = [vp, vp, i32, f32, ctypes.c_int64, vp, ctypes.c_int64, vp, vp]
    L.ldpc_decode_soft_typed.argtypes = [vp, vp, i32, f32, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, i32]
    L.ldpc_decode_soft_typed_device.argtypes = [vp, vp, i32, f32, ctypes.c_int64, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, i32, vp]
    L.ldpc_llr_quantize_device.argtypes = [vp, ctypes.c_int64, i32, f32, vp, i32, vp]
    L.ldpc_out_bytes.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]
    L.ldpc_out_bytes.restype = ctypes.c_int64
    L.ldpc_decoder_set_timing.argtypes = [vp, ctypes.c_int]
    L.ldpc_decoder_stats.argtypes = [vp, ctypes.POINTER(DecodeStats)]
    L.ldpc_decoder_kernel_times.argtypes = [vp, ctypes.POINTER(KernelTime), ctypes.c_int32, i32p]
    L.ldpc_decoder_set_tap.argtypes = [vp, ctypes.c_int32]
    L.ldpc_decoder_dump.argtypes = [vp, ctypes.c_int32, vp, ctypes.c_int64]
    L.ldpc_awgn_device.argtypes = [vp, ctypes.c_int64, ctypes.c_int32, vp, ctypes.c_float, ctypes.c_uint64,
                                   ctypes.c_int64, ctypes.c_int32, vp]
    L.ldpc_count_errors_device.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, i64p, ctypes.c_int32, vp]
    L.ldpc_hbm_sustained_device.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)]
    L.ldpc_hbm_probe_device.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                        ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.ldpc_host_block_plan.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                       ctypes.POINTER(ctypes.c_uint64)]
    L.ldpc_host_locked_ranges.argtypes = [i64p, i64p]
    L.ldpc_decoder_array_addresses.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.ldpc_decoder_placement.argtypes = [vp, i32p, i32p, ctypes.POINTER(ctypes.c_float)]
    L.ldpc_decoder_link_form.argtypes = [vp, i32p, i32p, ctypes.POINTER(ctypes.c_float)]
    L.ldpc_parity_structure.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, i32p]
    L.ldpc_encoder_create.argtypes = [vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(vp)]
    L.ldpc_encoder_destroy.argtypes = [vp]
    L.ldpc_encode_device.argtypes = [vp, vp, ctypes.c_int64, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32, vp]
    L.ldpc_encode.argtypes = [vp, vp, ctypes.c_int64, vp, ctypes.c_int64]
    L.ldpc_code_bytes.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]
    L.ldpc_code_bytes.restype = ctypes.c_int64
    rsp = ctypes.POINTER(RateSpec)
    L.ldpc_rate_spec_init.argtypes = [rsp, ctypes.c_int32]
    L.ldpc_rate_spec_init.restype = None
    L.ldpc_rate_lengths.argtypes = [rsp, i32p, i32p]
    L.ldpc_rate_index.argtypes = [rsp, ctypes.c_int32, ctypes.c_int32, vp]
    L.ldpc_rate_match_device.argtypes = [rsp, vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp,
                                         ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp]
    L.ldpc_rate_recover_device.argtypes = [rsp, vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int32, vp,
                                           ctypes.c_int32, vp]
    L.ldpc_rate_match.argtypes = [rsp, vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp,
                                  ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    L.ldpc_rate_recover.argtypes = [rsp, vp, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, vp, ctypes.c_int32, vp,
                                    ctypes.c_int32]
    msp = ctypes.POINTER(ModemSpec)
    L.ldpc_modem_spec_init.argtypes = [msp, ctypes.c_int32]
    L.ldpc_modem_spec_init.restype = None
    L.ldpc_modem_symbol_floats.argtypes = [msp, ctypes.c_int32]
    L.ldpc_modem_symbol_floats.restype = ctypes.c_int64
    L.ldpc_modem_index.argtypes = [msp, ctypes.c_int32, vp]
    L.ldpc_modem_points.argtypes = [ctypes.c_int32, vp]
    L.ldpc_modem_transmit_device.argtypes = [msp, vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_uint64,
                                             ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32, vp]
    L.ldpc_modem_demap_device.argtypes = [msp, vp, ctypes.c_int64, ctypes.c_int32, vp, ctypes.c_int32, vp]
    L.ldpc_modem_transmit.argtypes = [msp, vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.c_float, ctypes.c_uint64,
                                      ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32]
    L.ldpc_modem_demap.argtypes = [msp, vp, ctypes.c_int64, ctypes.c_int32, vp, ctypes.c_int32]
    tsp = ctypes.POINTER(TbSpec)
    L.ldpc_tb_spec_init.argtypes = [tsp, ctypes.c_int32, ctypes.c_int32]
    L.ldpc_tb_spec_init.restype = None
    L.ldpc_tb_layout.argtypes = [tsp, i32p]
    L.ldpc_crc_bits.argtypes = [ctypes.c_int32, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint32)]
    L.ldpc_tb_attach_device.argtypes = [tsp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32, vp]
    L.ldpc_tb_check_device.argtypes = [tsp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int32, vp]
    L.ldpc_tb_tally_device.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int64, i64p, ctypes.c_int32, vp]
    L.ldpc_tb_attach.argtypes = [tsp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32]
    L.ldpc_tb_check.argtypes = [tsp, vp, ctypes.c_int64, vp, vp, vp, ctypes.c_int32]
    L.ldpc_decoder_crc_stops.argtypes = [vp, i64p]
    L.ldpc_crc_weights.argtypes = [ctypes.c_int32, ctypes.c_int32, vp]
    L.ldpc_tb_frame_crc.argtypes = [tsp, i32p, i32p]
    bsp = ctypes.POINTER(BchSpec)
    L.ldpc_bch_spec_init.argtypes = [bsp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    L.ldpc_bch_spec_init.restype = None
    L.ldpc_bch_layout.argtypes = [bsp, i32p]
    L.ldpc_bch_generator.argtypes = [ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32, vp, ctypes.c_int32, i32p]
    L.ldpc_bch_encode_device.argtypes = [bsp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32, vp]
    L.ldpc_bch_decode_device.argtypes = [bsp, vp, ctypes.c_int64, vp, vp, ctypes.c_int32, vp]
    L.ldpc_bch_tally_device.argtypes = [vp, vp, vp, ctypes.c_int64, ctypes.c_int64, i64p, ctypes.c_int32, vp]
    L.ldpc_bch_encode.argtypes = [bsp, vp, ctypes.c_int64, vp, ctypes.c_int64, ctypes.c_int32]
    L.ldpc_bch_decode.argtypes = [bsp, vp, ctypes.c_int64, vp, vp, ctypes.c_int32]
    L.ldpc_osd_create.argtypes = [vp, i32, i32, i32, ctypes.POINTER(vp)]
    L.ldpc_osd_destroy.argtypes = [vp]
    L.ldpc_osd_device.argtypes = [vp, vp, ctypes.c_int64, i32, f32, vp, ctypes.c_int64, vp, vp, vp, vp]
    L.ldpc_osd_run.argtypes = [vp, vp, ctypes.c_int64, i32, f32, vp, ctypes.c_int64, vp, vp, vp]
    L.ldpc_osd_info.argtypes = [vp, i32p]
    L.ldpc_graph_systematic_order.argtypes = [vp, vp, i32p]
    L.ldpc_parity_dense.argtypes = [vp, i32, i64p]
    L.ldpc_parity_dense_rows.argtypes = [vp, i32, i32, i32, vp, ctypes.c_int64]
    L.ldpc_encoder_create_dense.argtypes = [vp, i32, i32, i32, ctypes.POINTER(vp)]
    L.ldpc_bp_fx_table.argtypes = [i32, i32p, i32, i32p]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise LdpcError(rc, load().ldpc_last_error().decode("utf-8", "replace"))

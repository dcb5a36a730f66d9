"""Thin Python objects over the C ABI (include/ldpc_hip.h): Graph, Decoder, Encoder, RateMatcher, Modem, Osd,
TransportBlock and BchCode.

Host-side plumbing only -- every decode runs in the HIP kernels of
libldpc_hip.so.  numpy arrays are passed as host pointers, integers (e.g. a
torch tensor's data_ptr()) as device pointers.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import DecoderConfig, DecodeStats, LdpcError  # noqa: F401

ALGO_SP, ALGO_MS, ALGO_LAYERED, ALGO_MS_FUSED, ALGO_LAYERED_HOST, ALGO_BP, ALGO_LAYERED_BP = 0, 1, 2, 3, 4, 5, 6
ALGO_LAYERED_FX, ALGO_LAYERED_BP_FX, ALGO_BITFLIP = 8, 9, 10   # 7 is not assigned
MSG_F32, MSG_F16, MSG_F8, MSG_I8 = 0, 1, 2, 4    # 3 is not assigned
PACK_BYTES, PACK_BITS = 0, 1
CODE_PACKED, CODE_BITS = 0, 1                              # enum ldpc_code_format
CODE_FORMATS = {"packed": CODE_PACKED, "bits": CODE_BITS}
PARITY_KINDS = {1: "dual_diagonal", 2: "staircase", 3: "dense"}        # enum ldpc_parity_kind
HOST_INPUT = {"auto": 0, "staged": 1, "lock_pages": 2}     # enum ldpc_host_input
SOFT_POSTERIOR, SOFT_EXTRINSIC = 1, 2                      # enum ldpc_soft_kind
SOFT_KINDS = {"posterior": SOFT_POSTERIOR, "extrinsic": SOFT_EXTRINSIC}
LLR_F32, LLR_F16, LLR_I8 = 0, 1, 2                         # enum ldpc_llr_type
LLR_TYPES = {"f32": LLR_F32, "f16": LLR_F16, "i8": LLR_I8}
LLR_DTYPES = {np.dtype(np.float32): LLR_F32, np.dtype(np.float16): LLR_F16, np.dtype(np.int8): LLR_I8}
ALGOS = {"sp": ALGO_SP, "ms": ALGO_MS, "layered": ALGO_LAYERED, "ms_fused": ALGO_MS_FUSED,
         "layered_host": ALGO_LAYERED_HOST, "bp": ALGO_BP, "layered_bp": ALGO_LAYERED_BP, "layered_fx": ALGO_LAYERED_FX,
         "layered_bp_fx": ALGO_LAYERED_BP_FX, "bitflip": ALGO_BITFLIP}

# two-bit fields of ldpc_decoder_config.tune_flags (enum ldpc_tune_field): True forces on, False off
TUNE_FIELDS = {"fused": 0, "ldsp": 2, "ldsp_ext": 4, "ldsp_pack": 6, "link_narrow": 8, "check_wide": 10,
               "syn_xcd": 12, "fused_pack": 14, "fused_loop": 16, "device_tail": 18, "merge": 20, "link_deep": 22, "link_half": 24,
               "link_guided": 26, "tiles_first": 28}
TUNE_ON_ONLY = {"fx_record": 30}      # LDPC_TUNE_FX_RECORD: on or absent (its "off" would not fit the int32 word)
TUNE_INTS = ("rows_per_wave", "cols_per_wave", "link_rows", "compact", "ldsp_grid", "ldsp_per_cu", "ldsp_waves", "place", "q_order")


def apply_tune(cfg, tune):
    """Fill the tuning fields of a DecoderConfig from a dict: tri-state names of TUNE_FIELDS
    (True / False / None = automatic), "fx_record" (True = on; False / None = off) and integers of TUNE_INTS (link_rows=-1: column-local fusion
    off; compact=-1: tail compaction off).  Kernel selection and launch shapes only."""
    flags, shape = 0, 0
    for k, v in (tune or {}).items():
        if k in TUNE_FIELDS:
            if v is not None:
                flags |= (1 if v else 2) << TUNE_FIELDS[k]
        elif k in TUNE_ON_ONLY:
            if v:
                flags |= 1 << TUNE_ON_ONLY[k]
        elif k == "ldsp_per_cu":
            shape |= int(v) & 255
        elif k == "ldsp_waves":
            shape |= (int(v) & 255) << 8
        elif k in TUNE_INTS:
            setattr(cfg, "tune_" + k, int(v))
        else:
            raise KeyError("unknown tuning field %r" % k)
    cfg.tune_flags, cfg.tune_ldsp_shape = flags, shape


def bp_fx_table(frac_bits):
    """The correction table of algo "layered_bp_fx" at `frac_bits` fractional bits (ldpc_bp_fx_table): int32, up to and
    including its first 0.  Needs no device."""
    L = _lib.load()
    n = ctypes.c_int32()
    _lib.check(L.ldpc_bp_fx_table(int(frac_bits), None, 0, ctypes.byref(n)))
    t = np.zeros(n.value, np.int32)
    _lib.check(L.ldpc_bp_fx_table(int(frac_bits), t.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), t.size, ctypes.byref(n)))
    return t


def hbm_probe(device=0, nbytes=1 << 30, reps=5, by_policy=False):
    """GB/s of a plain float4 copy on `device` (read + write), best of `reps` launches with the default
    cache policy and `reps` with non-temporal loads and stores; by_policy=True: (best, default, nt)."""
    g = ctypes.c_double(0.0)
    two = (ctypes.c_double * 2)(0.0, 0.0)
    _lib.check(_lib.load().ldpc_hbm_probe_device(int(device), int(nbytes), int(reps), ctypes.byref(g), two))
    return (g.value, two[0], two[1]) if by_policy else g.value


def hbm_sustained(device=0, nbytes=1 << 30, milliseconds=300):
    """GB/s of the non-temporal float4 copy run back to back for `milliseconds` (first third untimed)."""
    g = ctypes.c_double(0.0)
    _lib.check(_lib.load().ldpc_hbm_sustained_device(int(device), int(nbytes), int(milliseconds), ctypes.byref(g)))
    return g.value


def tune_from_env(env=None):
    """For the measurement scripts under tools/: translate LDPC_TUNE_* environment switches into
    a tuning dict for Decoder(tune=...).  The library itself reads no environment variables."""
    import os
    env = os.environ if env is None else env
    t = {}
    for name, key in (("FUSED", "fused"), ("LDSP", "ldsp"), ("LDSP_EXT", "ldsp_ext"), ("LDSP_PACK", "ldsp_pack"),
                      ("LINK_NARROW", "link_narrow"), ("CHECK_WIDE", "check_wide"), ("SYN_XCD", "syn_xcd"),
                      ("FUSED_LOOP", "fused_loop"), ("DEVICE_TAIL", "device_tail"), ("MERGE", "merge"), ("LINK_DEEP", "link_deep"), ("LINK_HALF", "link_half"),
                      ("LINK_GUIDED", "link_guided"), ("TILES_FIRST", "tiles_first"), ("FX_RECORD", "fx_record")):
        if "LDPC_TUNE_" + name in env:
            t[key] = int(env["LDPC_TUNE_" + name]) != 0
    if "LDPC_TUNE_NO_PACK" in env:
        t["fused_pack"] = False
    for name, key in (("RPW", "rows_per_wave"), ("CPW", "cols_per_wave"), ("LDSP_GRID", "ldsp_grid"),
                      ("LDSP_PER_CU", "ldsp_per_cu"), ("LDSP_WAVES", "ldsp_waves")):
        if "LDPC_TUNE_" + name in env:
            t[key] = int(env["LDPC_TUNE_" + name])
    for name, key in (("LINK_RPW", "link_rows"), ("COMPACT", "compact")):     # 0 meant "off"
        if "LDPC_TUNE_" + name in env:
            v = int(env["LDPC_TUNE_" + name])
            t[key] = v if v > 0 else -1
    return t


def shard_range(frames, part, parts, unit=1):
    """ldpc_shard_range: frames [lo, hi) of part `part` of `parts` (boundaries multiples of `unit`)."""
    lo, hi = ctypes.c_int64(), ctypes.c_int64()
    _lib.check(_lib.load().ldpc_shard_range(int(frames), int(part), int(parts), int(unit),
                                            ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def host_block_plan(base, frames, N, max_batch, group):
    """ldpc_host_block_plan: (s0, s1, b0, b1, body_end, whole_by_cpu) of launch group `group` in lock mode."""
    out = (ctypes.c_uint64 * 6)()
    _lib.check(_lib.load().ldpc_host_block_plan(int(base), int(frames), int(N), int(max_batch), int(group), out))
    return tuple(int(x) for x in out)


def host_locked_ranges():
    """(live, stale): ranges of caller memory the library holds page-locked now / failed to release."""
    a, b = ctypes.c_int64(-1), ctypes.c_int64(-1)
    _lib.check(_lib.load().ldpc_host_locked_ranges(ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def device_count():
    n = ctypes.c_int(0)
    rc = _lib.load().ldpc_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def quantize_device(y_ptr, count, llr_type, llr_unit, out_ptr, device=0, stream=None):
    """ldpc_llr_quantize_device: `count` float32 values at y_ptr -> int8 ("i8") or float16 ("f16") at out_ptr, the
    sender's side of a typed decode call: t = y / llr_unit, rounded to nearest even and clamped to [-127, 127] / +-65504
    (NaN -> 0 / NaN).  Device pointers; enqueued on `stream`, no wait."""
    _lib.check(_lib.load().ldpc_llr_quantize_device(y_ptr, int(count), LLR_TYPES.get(llr_type, llr_type), float(llr_unit), out_ptr,
                                                    int(device), stream))


def out_bytes(K, frames, pack_mode=PACK_BYTES):
    return int(_lib.load().ldpc_out_bytes(K, frames, pack_mode))


def code_bytes(N, frames, fmt="packed"):
    """ldpc_code_bytes: bytes of `frames` codewords (0: unknown format, or packed with N % 8 != 0)."""
    return int(_lib.load().ldpc_code_bytes(int(N), int(frames), CODE_FORMATS.get(fmt, fmt)))


def parity_structure(graph, K, block_rows=0):
    """ldpc_parity_structure: how the encoder would solve the parity part H[:, K..N) -- host analysis only.
    dict(kind="dual_diagonal" | "staircase", c, x, a, b, ext_rows, z); LdpcError code 4 for any other structure."""
    out = (ctypes.c_int32 * 8)()
    _lib.check(_lib.load().ldpc_parity_structure(graph._h, int(K), int(block_rows), out))
    return dict(kind=PARITY_KINDS[out[0]], c=out[1], x=out[2], a=out[3], b=out[4], ext_rows=out[5], z=out[6])


def systematic_order(graph):
    """ldpc_graph_systematic_order: (perm, rank) -- column perm[i] of H is column i of the re-ordered H', which is
    encodable with K = N - rank by DenseEncoder (codes.permute_columns applies perm).  Host only."""
    perm = np.zeros(graph.N, np.int32)
    rank = ctypes.c_int32(0)
    _lib.check(_lib.load().ldpc_graph_systematic_order(graph._h, perm.ctypes.data, ctypes.byref(rank)))
    return perm, rank.value


def dense_parity(graph, K):
    """ldpc_parity_dense: dict(rho, rank_hp, M, t_words) of the dense parity solve of H[:, K..N) -- host analysis only;
    LdpcError code 4 if the parity part is singular, the information bits are not free or M > 16384."""
    out = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().ldpc_parity_dense(graph._h, int(K), out))
    return dict(rho=out[0], rank_hp=out[1], M=out[2], t_words=out[3])


def dense_parity_rows(graph, K, first, rows):
    """ldpc_parity_dense_rows: uint64 [rows, ceil(M / 64)], rows [first, first + rows) of T with T H_p = I (bit j of a row =
    bit j % 64 of word j // 64)."""
    tw = (graph.M + 63) // 64
    out = np.zeros((max(int(rows), 0), tw), np.uint64)
    _lib.check(_lib.load().ldpc_parity_dense_rows(graph._h, int(K), int(first), int(rows), out.ctypes.data, out.size))
    return out


class Graph:
    """Parity-check matrix as its nonzeros in row-major order (edge id = rank),
    the form Coder::forDecoder builds at MyLdpc.cpp:171-222."""

    def __init__(self, rows, cols, M, N):
        L = _lib.load()
        self.rows = np.ascontiguousarray(rows, np.int32)
        self.cols = np.ascontiguousarray(cols, np.int32)
        if self.rows.shape != self.cols.shape or self.rows.ndim != 1:
            raise ValueError("rows and cols must be 1-D arrays of equal length")
        self.M, self.N, self.E = int(M), int(N), int(self.rows.size)
        self._h = ctypes.c_void_p()
        i32p = ctypes.POINTER(ctypes.c_int32)
        _lib.check(L.ldpc_graph_create(self.rows.ctypes.data_as(i32p), self.cols.ctypes.data_as(i32p),
                                       self.E, self.M, self.N, ctypes.byref(self._h)))

    def info(self):
        L = _lib.load()
        M, N, rd, cd = (ctypes.c_int32() for _ in range(4))
        E = ctypes.c_int64()
        _lib.check(L.ldpc_graph_info(self._h, ctypes.byref(M), ctypes.byref(N), ctypes.byref(E),
                                     ctypes.byref(rd), ctypes.byref(cd)))
        return dict(M=M.value, N=N.value, E=E.value, max_row_deg=rd.value, max_col_deg=cd.value)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:   # module may be torn down at exit
            _lib._lib.ldpc_graph_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Decoder:
    """One decoder handle = the device state Coder::forDecoder + addDecodeType set
    up (MyLdpc.cpp:226-552) for one algorithm."""

    def __init__(self, graph, K, max_batch, algo="sp", max_iter=40, llr_scale=8.0, early_term=True,
                 device=0, layer_rows=0, pack_mode=PACK_BYTES, frames_per_lane=0, poll_interval=0,
                 msg_dtype=MSG_F32, tune=None, devices=None, host_input="auto", host_copy_threads=0,
                 ms_scale=0.0, ms_offset=0.0, crc_kind=0, crc_bits=0, msg_bits=0, post_bits=0, bp_frac_bits=0,
                 bf_threshold=None):
        L = _lib.load()
        algo = ALGOS[algo] if isinstance(algo, str) else int(algo)
        # algo "bitflip" (hard-decision bit flipping): the struct with the sixteen round offsets behind it; bf_threshold is a
        # sequence of up to 16 offsets in [0, 62], the last one repeated (None or all zero: off(i) = i - 1).  Every other
        # algorithm keeps the struct it always passed
        bf = algo == ALGO_BITFLIP or bf_threshold is not None
        cfg = _lib.DecoderConfigBf() if bf else _lib.DecoderConfigMsg()
        _lib.check(L.ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)))
        if bf_threshold is not None:
            t = [int(v) for v in bf_threshold]
            if not 1 <= len(t) <= 16:
                raise ValueError("bf_threshold holds 1 to 16 round offsets")
            cfg.bf_threshold[:] = t + [t[-1]] * (16 - len(t))
        cfg.K, cfg.max_batch = int(K), int(max_batch)
        cfg.algo = algo
        cfg.msg_dtype = {"f32": MSG_F32, "f16": MSG_F16, "f8": MSG_F8, "i8": MSG_I8}.get(msg_dtype, msg_dtype)
        # fixed-point messages, msg_dtype "i8": saturating integers of msg_bits = 4, 5, 6 or 8 bits (0 = 8); llr_scale is
        # then the LSBs per unit of channel value (include/ldpc_hip.h: LDPC_MSG_I8)
        cfg.msg_bits = int(msg_bits)
        # algo "layered_fx" (msg_dtype "i8"): the posterior memory has post_bits bits, msg_bits <= post_bits <= 16 (0 = 16)
        cfg.post_bits = int(post_bits)
        # algo "layered_bp_fx" (msg_dtype "i8", msg_bits, post_bits as for "layered_fx"): box-plus rows from a correction table;
        # one LSB is 2^-bp_frac_bits LLR units (0 ... 4) and llr_scale * y is the channel LLR in LSBs
        cfg.bp_frac_bits = int(bp_frac_bits)
        cfg.max_iter, cfg.llr_scale = int(max_iter), float(llr_scale)
        cfg.early_term, cfg.device, cfg.layer_rows = int(bool(early_term)), int(device), int(layer_rows)
        cfg.pack_mode, cfg.frames_per_lane, cfg.poll_interval = int(pack_mode), int(frames_per_lane), int(poll_interval)
        apply_tune(cfg, tune)
        # how ldpc_decode() moves pageable channel values: through the library's pinned ring (default) or by
        # page-locking the caller's pages for the call (include/ldpc_hip.h: enum ldpc_host_input)
        cfg.host_input = HOST_INPUT[host_input] if isinstance(host_input, str) else int(host_input)
        cfg.host_copy_threads = int(host_copy_threads)
        # normalized / offset min-sum, algo "ms" / "layered": R = fmaxf(min - ms_offset, 0) * ms_scale (0 = off)
        cfg.ms_scale, cfg.ms_offset = float(ms_scale), float(ms_offset)
        # CRC-aided early termination: a frame also stops once its first crc_bits hard bits pass the CRC (0 = off;
        # kind 16, 24 (24A), 25 (24B) or "16" / "24a" / "24b"; TransportBlock.frame_crc() gives both)
        cfg.crc_kind, cfg.crc_bits = int(CRC_KINDS.get(crc_kind, crc_kind)), int(crc_bits)
        self.cfg = cfg
        self.graph = graph
        self.K, self.N, self.E = int(K), graph.N, graph.E
        self._h = ctypes.c_void_p()
        if devices is None:
            _lib.check(L.ldpc_decoder_create(graph._h, ctypes.byref(cfg), ctypes.byref(self._h)))
        else:       # one handle over several devices (ldpc_decoder_create_multi): host-buffer decode only
            devs = (ctypes.c_int32 * len(devices))(*[int(x) for x in devices])
            _lib.check(L.ldpc_decoder_create_multi(graph._h, ctypes.byref(cfg), devs, len(devices),
                                                   ctypes.byref(self._h)))

    # -- host buffers (the reference's Coder::decode signature) -------------
    def decode(self, llr, want_iters=True, soft=None, llr_unit=None):
        """llr: float32 [frames, N] (numpy).  Returns (bytes uint8, iters int32); with soft="posterior" or "extrinsic"
        (ldpc_decode_soft) a third value, float32 [frames, N]: per frame the posterior of the round it stopped in, or
        that minus the channel value.
        llr_unit: the typed path (ldpc_decode_typed / ldpc_decode_soft_typed) -- the element type is the array's own
        dtype, int8, float16 or float32 (unit exactly 1), and the decoder reads y = x * llr_unit.  Without llr_unit any
        array is converted to float32 first, as always."""
        L = _lib.load()
        if llr_unit is not None:
            llr = np.asarray(llr)
            if llr.dtype not in LLR_DTYPES:
                raise TypeError("llr_unit given: llr must be int8, float16 or float32, not %s" % llr.dtype)
            llr = np.ascontiguousarray(llr).reshape(-1, self.N)
            frames, ty = llr.shape[0], LLR_DTYPES[llr.dtype]
            out = np.zeros(out_bytes(self.K, frames, self.cfg.pack_mode), np.uint8)
            iters = np.zeros(frames, np.int32)
            if soft is None:
                _lib.check(L.ldpc_decode_typed(self._h, llr.ctypes.data, ty, float(llr_unit), frames, out.ctypes.data, out.size,
                                               iters.ctypes.data if want_iters else None))
                return out, iters
            vals = np.zeros((frames, self.N), np.float32)
            _lib.check(L.ldpc_decode_soft_typed(self._h, llr.ctypes.data, ty, float(llr_unit), frames, out.ctypes.data, out.size,
                                                iters.ctypes.data if want_iters else None, vals.ctypes.data, vals.size,
                                                SOFT_KINDS.get(soft, soft)))
            return out, iters, vals
        llr = np.ascontiguousarray(llr, np.float32).reshape(-1, self.N)
        frames = llr.shape[0]
        out = np.zeros(out_bytes(self.K, frames, self.cfg.pack_mode), np.uint8)
        iters = np.zeros(frames, np.int32)
        if soft is None:
            _lib.check(L.ldpc_decode(self._h, llr.ctypes.data, frames, out.ctypes.data, out.size,
                                     iters.ctypes.data if want_iters else None))
            return out, iters
        vals = np.zeros((frames, self.N), np.float32)
        _lib.check(L.ldpc_decode_soft(self._h, llr.ctypes.data, frames, out.ctypes.data, out.size,
                                      iters.ctypes.data if want_iters else None, vals.ctypes.data, vals.size,
                                      SOFT_KINDS.get(soft, soft)))
        return out, iters, vals

    # -- buffers already in HBM ----------------------------------------------
    def decode_device(self, llr_ptr, frames, out_ptr, out_nbytes, iters_ptr=None, stream=None, soft_ptr=None, soft_floats=0,
                      soft="posterior", llr_type=None, llr_unit=None):
        """ldpc_decode_device: out_ptr None = iteration counts and stats() only; iters_ptr None = bytes only.
        soft_ptr: ldpc_decode_soft_device -- soft_floats >= frames * N float32 values of kind `soft` are written there.
        llr_type ("f32", "f16", "i8") / llr_unit: ldpc_decode_typed_device / ldpc_decode_soft_typed_device -- llr_ptr holds
        elements of that type and the decoder reads y = x * llr_unit (default 1)."""
        if llr_type is not None or llr_unit is not None:
            ty = LLR_TYPES.get(llr_type, llr_type) if llr_type is not None else LLR_F32
            unit = 1.0 if llr_unit is None else float(llr_unit)
            if soft_ptr is None and not soft_floats:
                _lib.check(_lib.load().ldpc_decode_typed_device(self._h, llr_ptr, ty, unit, frames, out_ptr, out_nbytes, iters_ptr,
                                                                stream))
            else:
                _lib.check(_lib.load().ldpc_decode_soft_typed_device(self._h, llr_ptr, ty, unit, frames, out_ptr, out_nbytes,
                                                                     iters_ptr, soft_ptr, int(soft_floats),
                                                                     SOFT_KINDS.get(soft, soft), stream))
        elif soft_ptr is None and not soft_floats:
            _lib.check(_lib.load().ldpc_decode_device(self._h, llr_ptr, frames, out_ptr, out_nbytes,
                                                      iters_ptr, stream))
        else:
            _lib.check(_lib.load().ldpc_decode_soft_device(self._h, llr_ptr, frames, out_ptr, out_nbytes, iters_ptr, soft_ptr,
                                                           int(soft_floats), SOFT_KINDS.get(soft, soft), stream))

    def set_timing(self, enable=True):
        """True / 1: time every launch of every call; k > 1: of every k-th decode_device call; False: off."""
        _lib.check(_lib.load().ldpc_decoder_set_timing(self._h, int(enable)))

    def stats(self):
        st = DecodeStats()
        _lib.check(_lib.load().ldpc_decoder_stats(self._h, ctypes.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def crc_stops(self):
        """Frames of the last call stopped by the CRC in a round in which their syndrome was not clean."""
        n = ctypes.c_int64(0)
        _lib.check(_lib.load().ldpc_decoder_crc_stops(self._h, ctypes.byref(n)))
        return n.value

    def kernel_times(self):
        """Per-kernel HIP-event times gathered since set_timing(True)."""
        arr = (_lib.KernelTime * 64)()
        n = ctypes.c_int32(0)
        _lib.check(_lib.load().ldpc_decoder_kernel_times(self._h, arr, 64, ctypes.byref(n)))
        return [dict(name=arr[i].name.decode(), phase=arr[i].phase, degree=arr[i].degree,
                     launches=arr[i].launches, ms_total=arr[i].ms_total, bytes_total=arr[i].bytes_total,
                     bytes_moved=arr[i].bytes_moved)
                for i in range(n.value)]

    def link_form(self):
        """Form of the column-fused check kernel (None: the code has none) and the creation-time measurement."""
        form, cal = ctypes.c_int32(-1), ctypes.c_int32(0)
        ms = (ctypes.c_float * 3)()
        _lib.check(_lib.load().ldpc_decoder_link_form(self._h, ctypes.byref(form), ctypes.byref(cal), ms))
        if form.value < 0:
            return None
        return {"form": ("wide", "narrow", "half")[form.value], "chosen_by_measurement": bool(cal.value),
                "ms_per_launch": {"wide": round(ms[0], 4), "narrow": round(ms[1], 4), "half": round(ms[2], 4)}}

    def placement(self):
        """The creation-time placement search: per candidate set of arrays the column-fused check kernel's time per
        launch, and which one was kept (None: no search was made)."""
        n, kept = ctypes.c_int32(0), ctypes.c_int32(0)
        ms = (ctypes.c_float * 16)()
        _lib.check(_lib.load().ldpc_decoder_placement(self._h, ctypes.byref(n), ctypes.byref(kept), ms))
        if n.value == 0:
            return None
        return {"candidates_ms": [round(ms[i], 4) for i in range(n.value)], "kept": kept.value}

    def array_addresses(self):
        """Device addresses of the streaming decoder's Q, R, channel and hard-bit arrays."""
        a = (ctypes.c_uint64 * 4)()
        _lib.check(_lib.load().ldpc_decoder_array_addresses(self._h, a))
        return {"Q": int(a[0]), "R": int(a[1]), "chan": int(a[2]), "hard": int(a[3])}

    def set_tap(self, it):
        _lib.check(_lib.load().ldpc_decoder_set_tap(self._h, int(it)))

    def dump(self, which, frames):
        per = self.N if which in (2, 3) else self.E
        if self.cfg.algo == ALGO_BITFLIP and which == 0:        # the syndrome words, one value per row
            per = self.graph.M
        a = np.empty((frames, per), np.float32)
        _lib.check(_lib.load().ldpc_decoder_dump(self._h, which, a.ctypes.data, a.size))
        return a

    def close(self):
        """ldpc_decoder_destroy; raises if the library reports page-locked blocks it could not release."""
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:
            _lib.check(_lib._lib.ldpc_decoder_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Encoder:
    """One encoder handle (ldpc_encoder_create): systematic encoding of up to `max_frames` frames per call in HIP
    kernels, data conventions of Coder::encode.  block_rows: circulant size z of a quasi-cyclic code (0: staircase
    codes).  There is no CPU path: without a device the constructor raises LdpcError code 2."""

    def __init__(self, graph, K, block_rows=0, max_frames=4096, device=0):
        self.graph, self.K, self.N = graph, int(K), graph.N
        self.block_rows, self.max_frames, self.device = int(block_rows), int(max_frames), int(device)
        self._h = ctypes.c_void_p()
        _lib.check(self._create(_lib.load()))

    def _create(self, L):
        return L.ldpc_encoder_create(self.graph._h, self.K, self.block_rows, self.max_frames, self.device, ctypes.byref(self._h))

    def structure(self):
        return parity_structure(self.graph, self.K, self.block_rows)

    def encode(self, src_bytes):
        """Host buffers: the source byte stream (bytes / uint8 array) -> packed codewords, uint8 [frames * N/8];
        the frame count follows from the length as in Coder::encode."""
        src = np.ascontiguousarray(np.frombuffer(bytes(src_bytes), np.uint8) if isinstance(src_bytes, (bytes, bytearray))
                                   else src_bytes, np.uint8).reshape(-1)
        frames = 1
        while frames * self.K // 8 < src.size:
            frames += 1
        out = np.zeros(code_bytes(self.N, frames, "packed"), np.uint8)
        _lib.check(_lib.load().ldpc_encode(self._h, src.ctypes.data, src.size, out.ctypes.data, out.size))
        return out

    def encode_device(self, src_ptr, src_nbytes, frames, code_ptr, code_nbytes, fmt="bits", stream=None):
        """Buffers already in HBM (integers, e.g. a torch tensor's data_ptr()); enqueued on `stream`, no wait."""
        _lib.check(_lib.load().ldpc_encode_device(self._h, src_ptr, int(src_nbytes), int(frames), code_ptr,
                                                  int(code_nbytes), CODE_FORMATS.get(fmt, fmt), stream))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:
            _lib.check(_lib._lib.ldpc_encoder_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DenseEncoder(Encoder):
    """An encoder handle for any H (ldpc_encoder_create_dense): the parity bits are the solution of H_p p = H_s u by a
    dense GF(2) product on the device; encode / encode_device are Encoder's.  H[:, K..N) must have full column rank and
    rank(H) = N - K: systematic_order + codes.permute_columns make any H so.  LdpcError code 4 otherwise, code 2 without
    a device."""

    def __init__(self, graph, K, max_frames=4096, device=0):
        super().__init__(graph, K, 0, max_frames, device)

    def _create(self, L):
        return L.ldpc_encoder_create_dense(self.graph._h, self.K, self.max_frames, self.device, ctypes.byref(self._h))

    def structure(self):
        return dict(dense_parity(self.graph, self.K), kind="dense")


class RateMatcher:
    """Rate matching between the encoder and the decoders (ldpc_rate_*, include/ldpc_hip.h): puncturing of the first
    `punctured` code bits, filler bits [filler[0], filler[1]) that are known zeros, a transmission (k0, E) read from the
    circular buffer, repetition for E > L and soft combining of retransmissions.  A plain parameter set: no handle.
    erasure_llr: 0 = never-received positions read 0.0; 1e-6 whenever a layered decoder reads `y` (the header says why)."""

    def __init__(self, N, punctured=0, filler=(0, 0), fill_llr=10.0, erasure_llr=0.0, device=0):
        L = _lib.load()
        self.spec = _lib.RateSpec()
        L.ldpc_rate_spec_init(ctypes.byref(self.spec), int(N))
        self.spec.punctured = int(punctured)
        self.spec.filler_lo, self.spec.filler_hi = int(filler[0]), int(filler[1])
        self.spec.fill_llr, self.spec.erasure_llr = float(fill_llr), float(erasure_llr)
        self.N, self.device = int(N), int(device)
        self.lengths()      # an unusable spec fails here

    def lengths(self):
        """(Ncb, L): circular-buffer positions and the transmittable ones among them."""
        ncb, l = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(_lib.load().ldpc_rate_lengths(ctypes.byref(self.spec), ctypes.byref(ncb), ctypes.byref(l)))
        return ncb.value, l.value

    def index(self, k0, E):
        """int32 [E]: the code bit behind each transmitted position (host arithmetic only)."""
        out = np.zeros(max(int(E), 0), np.int32)
        _lib.check(_lib.load().ldpc_rate_index(ctypes.byref(self.spec), int(k0), int(E), out.ctypes.data))
        return out

    # -- buffers already in HBM (integers, e.g. a torch tensor's data_ptr()); enqueued on `stream`, no wait --------
    def match_device(self, code_ptr, frames, k0, E, tx_ptr, tx_nbytes, code_fmt="bits", tx_fmt="bits", stream=None):
        _lib.check(_lib.load().ldpc_rate_match_device(ctypes.byref(self.spec), code_ptr, CODE_FORMATS.get(code_fmt, code_fmt),
                                                      int(frames), int(k0), int(E), tx_ptr, int(tx_nbytes),
                                                      CODE_FORMATS.get(tx_fmt, tx_fmt), self.device, stream))

    def recover_device(self, rx_ptr, frames, k0, E, soft_ptr=None, accumulate=False, y_ptr=None, stream=None):
        _lib.check(_lib.load().ldpc_rate_recover_device(ctypes.byref(self.spec), rx_ptr, int(frames), int(k0), int(E), soft_ptr,
                                                        int(bool(accumulate)), y_ptr, self.device, stream))

    # -- host buffers (numpy); blocking ---------------------------------------------------------------------------
    def match(self, code, k0, E, code_fmt="bits", tx_fmt="bits"):
        """code: uint8 [frames, N] (bits) or [frames, N/8] (packed) -> uint8 [frames, E] or [frames, E/8]."""
        per_in = self.N if code_fmt == "bits" else self.N // 8
        code = np.ascontiguousarray(code, np.uint8).reshape(-1, per_in)
        frames = code.shape[0]
        per_out = int(E) if tx_fmt == "bits" else int(E) // 8
        tx = np.zeros((frames, max(per_out, 0)), np.uint8)
        _lib.check(_lib.load().ldpc_rate_match(ctypes.byref(self.spec), code.ctypes.data, CODE_FORMATS.get(code_fmt, code_fmt), frames,
                                               int(k0), int(E), tx.ctypes.data, tx.size, CODE_FORMATS.get(tx_fmt, tx_fmt), self.device))
        return tx

    def recover(self, rx, k0, E, soft=None, want_y=True):
        """rx: float32 [frames, E].  soft: None, or float32 [frames, N] that is accumulated into IN PLACE.
        Returns (soft, y); without `soft` the sums of this transmission alone are returned as a new array."""
        rx = np.ascontiguousarray(rx, np.float32).reshape(-1, int(E))
        frames = rx.shape[0]
        accumulate = soft is not None
        if soft is None:
            soft = np.zeros((frames, self.N), np.float32)
        assert soft.dtype == np.float32 and soft.flags.c_contiguous and soft.size == frames * self.N
        y = np.zeros((frames, self.N), np.float32) if want_y else None
        _lib.check(_lib.load().ldpc_rate_recover(ctypes.byref(self.spec), rx.ctypes.data, frames, int(k0), int(E), soft.ctypes.data,
                                                 int(accumulate), None if y is None else y.ctypes.data, self.device))
        return soft, y


class Modem:
    """The modem stage between RateMatcher.match and RateMatcher.recover (ldpc_modem_*, include/ldpc_hip.h): bit
    interleaver, Gray mapper (Qm = 1: the reference's BPSK, 2: QPSK, 4 / 6 / 8: 16-, 64-, 256-QAM at unit mean energy),
    AWGN of standard deviation `sd` per real dimension from the counter-based generator, and the max-log demapper, whose
    output is in the decoders' units (true LLR = 2 y / sd^2; a sum-product decoder wants llr_scale = 2 / sd^2).
    interleave: None = the library's default (on for Qm >= 2).  A plain parameter set: no handle."""

    def __init__(self, Qm, interleave=None, device=0):
        L = _lib.load()
        self.spec = _lib.ModemSpec()
        L.ldpc_modem_spec_init(ctypes.byref(self.spec), int(Qm))
        if interleave is not None:
            self.spec.interleave = int(bool(interleave))
        self.Qm, self.device = int(Qm), int(device)
        self.points()       # an unusable Qm fails here

    def symbol_floats(self, E):
        """Floats of one frame's row of symbols: E for Qm = 1, else 2 E / Qm."""
        n = int(_lib.load().ldpc_modem_symbol_floats(ctypes.byref(self.spec), int(E)))
        if n == 0:
            _lib.check(1)
        return n

    def index(self, E):
        """int32 [E]: entry j * Qm + i is the tx bit that becomes bit i of symbol j (host arithmetic only)."""
        out = np.zeros(max(int(E), 0), np.int32)
        _lib.check(_lib.load().ldpc_modem_index(ctypes.byref(self.spec), int(E), out.ctypes.data))
        return out

    def points(self):
        """float32 [2^Qm, 2]: (I, Q) of every label v = sum b_i 2^(Qm-1-i)."""
        out = np.zeros((1 << max(min(self.Qm, 8), 0), 2), np.float32)
        _lib.check(_lib.load().ldpc_modem_points(self.Qm, out.ctypes.data))
        return out

    # -- buffers already in HBM (integers, e.g. a torch tensor's data_ptr()); enqueued on `stream`, no wait --------
    def transmit_device(self, tx_ptr, frames, E, sd, seed, sym_ptr, sym_floats, first_frame=0, tx_fmt="bits", stream=None):
        _lib.check(_lib.load().ldpc_modem_transmit_device(ctypes.byref(self.spec), tx_ptr, CODE_FORMATS.get(tx_fmt, tx_fmt), int(frames),
                                                          int(E), float(sd), int(seed), int(first_frame), sym_ptr, int(sym_floats),
                                                          self.device, stream))

    def demap_device(self, sym_ptr, frames, E, rx_ptr, stream=None):
        _lib.check(_lib.load().ldpc_modem_demap_device(ctypes.byref(self.spec), sym_ptr, int(frames), int(E), rx_ptr, self.device, stream))

    # -- host buffers (numpy); blocking ---------------------------------------------------------------------------
    def transmit(self, tx, sd, seed, first_frame=0, tx_fmt="bits"):
        """tx: uint8 [frames, E] (bits) or [frames, E/8] (packed) -> float32 [frames, symbol_floats(E)]."""
        tx = np.ascontiguousarray(tx, np.uint8)
        assert tx.ndim == 2
        frames, E = tx.shape[0], tx.shape[1] * (1 if tx_fmt == "bits" else 8)
        sym = np.zeros((frames, self.symbol_floats(E)), np.float32)
        _lib.check(_lib.load().ldpc_modem_transmit(ctypes.byref(self.spec), tx.ctypes.data, CODE_FORMATS.get(tx_fmt, tx_fmt), frames, E,
                                                   float(sd), int(seed), int(first_frame), sym.ctypes.data, sym.size, self.device))
        return sym

    def demap(self, sym, E):
        """sym: float32 [frames, symbol_floats(E)] -> float32 [frames, E], de-interleaved."""
        sym = np.ascontiguousarray(sym, np.float32).reshape(-1, self.symbol_floats(E))
        rx = np.zeros((sym.shape[0], int(E)), np.float32)
        _lib.check(_lib.load().ldpc_modem_demap(ctypes.byref(self.spec), sym.ctypes.data, sym.shape[0], int(E), rx.ctypes.data, self.device))
        return rx


CRC_KINDS = {"16": 16, "24a": 24, "24b": 25}               # enum ldpc_crc_kind


class TransportBlock:
    """The transport-block stage in front of Encoder.encode_device and behind Decoder.decode_device (ldpc_tb_*,
    include/ldpc_hip.h): a CRC on the A payload bits (tb_crc 0, 16 or 24 = CRC24A), segmentation into C code blocks that
    each carry CRC24B (cb_crc 0 or 24), zero filler bits up to the code's K; at the receiver the CRC checks and the
    reassembly.  C, tb_crc, cb_crc: None = the rule of ldpc_tb_spec_init (TS 38.212 section 5.2.2 with K for Kcb).
    Frame t * C + c is code block c of transport block t.  A plain parameter set: no handle."""

    def __init__(self, A, K, C=None, tb_crc=None, cb_crc=None, device=0):
        L = _lib.load()
        self.spec = _lib.TbSpec()
        L.ldpc_tb_spec_init(ctypes.byref(self.spec), int(A), int(K))
        for name, v in (("C", C), ("tb_crc", tb_crc), ("cb_crc", cb_crc)):
            if v is not None:
                setattr(self.spec, name, int(v))
        self.device = int(device)
        self.B, self.S, self.Kp, self.filler_lo, self.filler_hi, self.C = self.layout()      # an unusable spec fails here
        self.A, self.K, self.tb_crc, self.cb_crc = self.spec.A, self.spec.K, self.spec.tb_crc, self.spec.cb_crc

    def layout(self):
        """(B, S, Kp, filler_lo, filler_hi, C): stream bits, bits per code block, bits in front of the fillers [Kp, K)."""
        out = (ctypes.c_int32 * 6)()
        _lib.check(_lib.load().ldpc_tb_layout(ctypes.byref(self.spec), out))
        return tuple(int(v) for v in out)

    @staticmethod
    def crc_bits(kind, data, nbits=None):
        """CRC of the first `nbits` bits (default: all) of a uint8 row in the project's bit order; kind: 16, 24 (24A),
        25 (24B) or "16" / "24a" / "24b".  Host arithmetic only."""
        data = np.ascontiguousarray(data, np.uint8).reshape(-1)
        n = data.size * 8 if nbits is None else int(nbits)
        assert n <= data.size * 8
        crc = ctypes.c_uint32()
        _lib.check(_lib.load().ldpc_crc_bits(CRC_KINDS.get(kind, kind), data.ctypes.data if data.size else None, n, ctypes.byref(crc)))
        return crc.value

    @staticmethod
    def crc_weights(kind, nbits):
        """uint32 [nbits]: entry n is the CRC of the unit vector e_n of nbits bits (ldpc_crc_weights); the XOR of the
        weights of a row's set bits is the row's CRC.  Host arithmetic only."""
        w = np.zeros(max(int(nbits), 0), np.uint32)
        _lib.check(_lib.load().ldpc_crc_weights(CRC_KINDS.get(kind, kind), int(nbits), w.ctypes.data if w.size else None))
        return w

    def frame_crc(self):
        """(crc_kind, crc_bits) of the CRC every frame carries, for Decoder(crc_kind=, crc_bits=): CRC24B over Kp bits
        with a code-block CRC, the transport block's CRC when C = 1; LdpcError code 1 when the frames have none."""
        kind, bits = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(_lib.load().ldpc_tb_frame_crc(ctypes.byref(self.spec), ctypes.byref(kind), ctypes.byref(bits)))
        return kind.value, bits.value

    # -- buffers already in HBM (integers, e.g. a torch tensor's data_ptr()); enqueued on `stream`, no wait --------
    def attach_device(self, payload_ptr, tbs, src_ptr, src_nbytes, stream=None):
        _lib.check(_lib.load().ldpc_tb_attach_device(ctypes.byref(self.spec), payload_ptr, int(tbs), src_ptr, int(src_nbytes),
                                                     self.device, stream))

    def check_device(self, dec_ptr, tbs, payload_ptr=None, cb_ok_ptr=None, tb_ok_ptr=None, stream=None):
        _lib.check(_lib.load().ldpc_tb_check_device(ctypes.byref(self.spec), dec_ptr, int(tbs), payload_ptr, cb_ok_ptr, tb_ok_ptr,
                                                    self.device, stream))

    def tally_device(self, tb_ok_ptr, payload_ptr, ref_ptr, tbs, stream=None):
        """Blocks.  (failed, wrong, undetected, parity_only) over `tbs` transport blocks of A/8 payload bytes."""
        counts = (ctypes.c_int64 * 4)()
        _lib.check(_lib.load().ldpc_tb_tally_device(tb_ok_ptr, payload_ptr, ref_ptr, int(tbs), self.A // 8, counts, self.device, stream))
        return tuple(int(v) for v in counts)

    # -- host buffers (numpy); blocking ---------------------------------------------------------------------------
    def attach(self, payload):
        """payload: uint8 [tbs, A/8] -> uint8 [tbs * C, K/8], the source rows of the encoder."""
        payload = np.ascontiguousarray(payload, np.uint8).reshape(-1, self.A // 8)
        tbs = payload.shape[0]
        src = np.zeros((tbs * self.C, self.K // 8), np.uint8)
        _lib.check(_lib.load().ldpc_tb_attach(ctypes.byref(self.spec), payload.ctypes.data, tbs, src.ctypes.data, src.size, self.device))
        return src

    def check(self, dec):
        """dec: uint8 [tbs * C, K/8] -> (payload uint8 [tbs, A/8], cb_ok uint8 [tbs * C], tb_ok uint8 [tbs])."""
        dec = np.ascontiguousarray(dec, np.uint8).reshape(-1, self.K // 8)
        assert dec.shape[0] % self.C == 0
        tbs = dec.shape[0] // self.C
        payload = np.zeros((tbs, self.A // 8), np.uint8)
        cb_ok, tb_ok = np.zeros(tbs * self.C, np.uint8), np.zeros(tbs, np.uint8)
        _lib.check(_lib.load().ldpc_tb_check(ctypes.byref(self.spec), dec.ctypes.data, tbs, payload.ctypes.data, cb_ok.ctypes.data,
                                             tb_ok.ctypes.data, self.device))
        return payload, cb_ok, tb_ok


class BchCode:
    """The outer code in front of Encoder.encode_device and behind Decoder.decode_device (ldpc_bch_*, include/ldpc_hip.h):
    a binary BCH code of n bits that corrects up to t errors, over GF(2^m) = GF(2)[x] / prim; m, prim: None = the rule
    of ldpc_bch_spec_init (m = 14 / 0x402B up to n = 16383, else m = 16 / 0x1002D).  Rows of row_bytes bytes (None:
    n / 8) hold the k = n - r message bits, the r parity bits and zeros.  A plain parameter set: no handle."""

    def __init__(self, n, t, row_bytes=None, m=None, prim=None, device=0):
        L = _lib.load()
        self.spec = _lib.BchSpec()
        L.ldpc_bch_spec_init(ctypes.byref(self.spec), int(n), int(t), int(n) // 8 if row_bytes is None else int(row_bytes))
        if m is not None:
            self.spec.m = int(m)
        if prim is not None:
            self.spec.prim = int(prim)
        self.device = int(device)
        self.k, self.r, self.nmin, self.m = self.layout()                     # an unusable spec fails here
        self.n, self.t, self.row_bytes, self.prim = self.spec.n, self.spec.t, self.spec.row_bytes, self.spec.prim

    def layout(self):
        """(k, r, number of distinct minimal polynomials, m)."""
        out = (ctypes.c_int32 * 4)()
        _lib.check(_lib.load().ldpc_bch_layout(ctypes.byref(self.spec), out))
        return tuple(int(v) for v in out)

    @staticmethod
    def generator_of(m, prim, t):
        """uint8 [r + 1]: the coefficients g_0 .. g_r of the generator of any valid (m, prim, t).  Host arithmetic only."""
        r = ctypes.c_int32()
        _lib.check(_lib.load().ldpc_bch_generator(int(m), int(prim), int(t), None, 0, ctypes.byref(r)))
        g = np.zeros(r.value + 1, np.uint8)
        _lib.check(_lib.load().ldpc_bch_generator(int(m), int(prim), int(t), g.ctypes.data, g.size, None))
        return g

    def generator(self):
        return self.generator_of(self.m, self.prim, self.t)

    # -- buffers already in HBM (integers, e.g. a torch tensor's data_ptr()); enqueued on `stream`, no wait --------
    def encode_device(self, payload_ptr, frames, src_ptr, src_nbytes, stream=None):
        _lib.check(_lib.load().ldpc_bch_encode_device(ctypes.byref(self.spec), payload_ptr, int(frames), src_ptr, int(src_nbytes),
                                                      self.device, stream))

    def decode_device(self, dec_ptr, frames, payload_ptr=None, status_ptr=None, stream=None):
        _lib.check(_lib.load().ldpc_bch_decode_device(ctypes.byref(self.spec), dec_ptr, int(frames), payload_ptr, status_ptr,
                                                      self.device, stream))

    def tally_device(self, status_ptr, payload_ptr, ref_ptr, frames, stream=None):
        """Blocks.  (failed, wrong, miscorrected_or_undetected, corrected_frames, corrected_bits, failed_though_equal)
        over `frames` frames of k/8 payload bytes."""
        counts = (ctypes.c_int64 * 6)()
        _lib.check(_lib.load().ldpc_bch_tally_device(status_ptr, payload_ptr, ref_ptr, int(frames), self.k // 8, counts, self.device, stream))
        return tuple(int(v) for v in counts)

    # -- host buffers (numpy); blocking ---------------------------------------------------------------------------
    def encode(self, payload):
        """payload: uint8 [frames, k/8] -> uint8 [frames, row_bytes], the source rows of the encoder."""
        payload = np.ascontiguousarray(payload, np.uint8).reshape(-1, self.k // 8)
        frames = payload.shape[0]
        src = np.zeros((frames, self.row_bytes), np.uint8)
        _lib.check(_lib.load().ldpc_bch_encode(ctypes.byref(self.spec), payload.ctypes.data, frames, src.ctypes.data, src.size, self.device))
        return src

    def decode(self, dec):
        """dec: uint8 [frames, row_bytes] -> (payload uint8 [frames, k/8], status int32 [frames])."""
        dec = np.ascontiguousarray(dec, np.uint8).reshape(-1, self.row_bytes)
        frames = dec.shape[0]
        payload = np.zeros((frames, self.k // 8), np.uint8)
        status = np.zeros(frames, np.int32)
        _lib.check(_lib.load().ldpc_bch_decode(ctypes.byref(self.spec), dec.ctypes.data, frames, payload.ctypes.data, status.ctypes.data,
                                               self.device))
        return payload, status


class Osd:
    """Ordered-statistics post-processing behind Decoder.decode_device(soft_ptr=...) (ldpc_osd_*, include/ldpc_hip.h): the
    frames whose hard decision (posterior < 0) has a dirty syndrome are re-encoded from their most reliable independent
    positions (order 0), with every single flip among them tried (order 1).  Codes up to N = 4096 and
    M * ceil(N / 32) <= 28672 words; LdpcError code 4 beyond.  On a machine without a device the handle is still made and
    the compute calls raise code 2 after their argument checks."""

    def __init__(self, graph, K, max_frames=4096, device=0):
        L = _lib.load()
        self.graph, self.K, self.N = graph, int(K), graph.N
        self.max_frames, self.device = int(max_frames), int(device)
        self._h = ctypes.c_void_p()
        _lib.check(L.ldpc_osd_create(graph._h, self.K, self.max_frames, self.device, ctypes.byref(self._h)))

    def info(self):
        """dict(M, N, words_per_row, lds_bytes): the dense image's shape and one workgroup's LDS."""
        out = (ctypes.c_int32 * 4)()
        _lib.check(_lib.load().ldpc_osd_info(self._h, out))
        return dict(M=out[0], N=out[1], words_per_row=out[2], lds_bytes=out[3])

    def run_device(self, soft_ptr, frames, order=1, weight_scale=256.0, out_ptr=None, out_nbytes=0, code_ptr=None, status_ptr=None,
                   metric_ptr=None, stream=None):
        """Buffers already in HBM (integers, e.g. a torch tensor's data_ptr()); enqueued on `stream`, no wait."""
        _lib.check(_lib.load().ldpc_osd_device(self._h, soft_ptr, int(frames), int(order), float(weight_scale), out_ptr, int(out_nbytes),
                                               code_ptr, status_ptr, metric_ptr, stream))

    def run(self, soft, order=1, weight_scale=256.0):
        """soft: float32 [frames, N] -> (out uint8 [frames, K/8] or None when K % 8 != 0, code uint8 [frames, N],
        status int32 [frames], metric int32 [frames]).  Host buffers, blocking, any number of frames."""
        soft = np.ascontiguousarray(soft, np.float32).reshape(-1, self.N)
        frames = soft.shape[0]
        out = np.zeros((frames, self.K // 8), np.uint8) if self.K % 8 == 0 else None
        code = np.zeros((frames, self.N), np.uint8)
        status, metric = np.zeros(frames, np.int32), np.zeros(frames, np.int32)
        _lib.check(_lib.load().ldpc_osd_run(self._h, soft.ctypes.data, frames, int(order), float(weight_scale),
                                            None if out is None else out.ctypes.data, 0 if out is None else out.size, code.ctypes.data,
                                            status.ctypes.data, metric.ctypes.data))
        return out, code, status, metric

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None and _lib._lib is not None:
            _lib.check(_lib._lib.ldpc_osd_destroy(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

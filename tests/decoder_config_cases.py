"""The configurations of the refusal sweep (test_decoder_config_cpu.py): pure data and loops, no randomness.

On the (648, 324) WiMAX graph, for every algo in 0..11 and every msg_dtype in 0..4: the base configuration, then every
single change of CHANGES and every pair of changes that do not set the same field.  (crc_bits = 328 lies behind K = 324
and is refused for that; crc 16/200 is the accepted value that lets the CRC rule's own refusals be reached.)  Every case
asks for a device no machine has, so a configuration that passes validation stops at the device check with LDPC_ERR_HIP
before anything is allocated, with or without a GPU.

The expected answers are tests/golden/decoder_config_refusals.npz.  They were recorded ONCE, from the library of the
commit in front of the one that moved validation into csrc/decoder_config_host.hpp (`python tests/decoder_config_cases.py
path/to/that/libldpc_hip.so out.npz`), and are what that library answered: the test compares the current library with
them byte for byte.  Recording them again from the library under test would only compare the library with itself; a case
list that has to change gets its fixture from a build of that earlier commit again.

Fixture layout: `messages` (the distinct refusal texts), `index[case]` (into messages, -1 = passed validation and was
stopped by the device check), `code[case]` (the LDPC_* code) and `names_sha256` (of the case names, so that a changed
case list cannot be compared with answers to another one).
"""
import ctypes
import hashlib
import itertools
import math

NO_DEVICE = 1 << 20
LDPC_ERR_HIP = 2
N, K, Z = 648, 324, 27          # codes.RATE_1_2: K = M = 324, circulant size 27
ALGOS = tuple(range(12))        # 7 and 11 are not assigned
MSG_DTYPES = tuple(range(5))    # 3 is not assigned

# the tuning word: two bits per field (1 on, 2 off, 3 no value), LDPC_TUNE_FUSED at bit 0, LDPC_TUNE_LDSP at bit 2,
# LDPC_TUNE_FX_RECORD bit 30
FUSED_ON, FUSED_OFF, LDSP_ON, LDSP_OFF, FX_RECORD = 1, 2, 1 << 2, 2 << 2, 1 << 30
# sizeof(ldpc_decoder_config) as it was before ms_scale, crc_kind, msg_bits and bf_threshold were appended
HISTORICAL_SIZES = (96, 104, 112, 128)
WRONG_SIZE = 100

# (name, field or fields it sets, values)
CHANGES = (
    [("msg_bits=%d" % v, {"msg_bits": v}) for v in (4, 7)] +
    [("post_bits=%d" % v, {"post_bits": v}) for v in (3, 12)] +
    [("bp_frac_bits=%d" % v, {"bp_frac_bits": v}) for v in (2, 99)] +
    [("ms_scale=0.75", {"ms_scale": 0.75}), ("ms_offset=nan", {"ms_offset": math.nan})] +
    [("llr_scale=%s" % v, {"llr_scale": v}) for v in (0.0, math.inf)] +
    [("layer_rows=%d" % v, {"layer_rows": v}) for v in (0, 27, 5)] +
    [("bf_threshold[0]=%d" % v, {"bf_threshold0": v}) for v in (3, 64)] +
    [("crc=%d/%d" % kb, {"crc_kind": kb[0], "crc_bits": kb[1]}) for kb in ((16, 328), (16, 16), (17, 328), (16, 200))] +
    [("early_term=0", {"early_term": 0}), ("frames_per_lane=3", {"frames_per_lane": 3}), ("pack_mode=5", {"pack_mode": 5})] +
    [("fused_on", {"tune_flags": FUSED_ON}), ("ldsp_on", {"tune_flags": LDSP_ON}), ("fused_on_ldsp_off", {"tune_flags": FUSED_ON | LDSP_OFF}),
     ("fx_record", {"tune_flags": FX_RECORD}), ("tune_field=3", {"tune_flags": 3})] +
    [("struct_size=%d" % v, {"struct_size": v}) for v in HISTORICAL_SIZES + (WRONG_SIZE,)]
)


def cases():
    """(name, dict of field -> value on top of the base configuration), in a fixed order"""
    for algo in ALGOS:
        for dt in MSG_DTYPES:
            head = "algo=%d msg_dtype=%d" % (algo, dt)
            yield head, {"algo": algo, "msg_dtype": dt}
            for name, ch in CHANGES:
                yield "%s %s" % (head, name), dict(ch, algo=algo, msg_dtype=dt)
            for (na, a), (nb, b) in itertools.combinations(CHANGES, 2):
                if set(a) & set(b):
                    continue            # two values of one field
                yield "%s %s %s" % (head, na, nb), dict(a, **b, algo=algo, msg_dtype=dt)


def names_sha256():
    h = hashlib.sha256()
    for name, _ in cases():
        h.update(name.encode() + b"\n")
    return h.hexdigest()


def graph():
    import myldpccppapi_amd as L
    from myldpccppapi_amd import codes
    assert codes.wimax_dims(codes.RATE_1_2, N) == (K, K, Z)
    return L.Graph(*codes.wimax_edges(codes.RATE_1_2, N), K, N)


def answers(lib, g):
    """[(code, message or None when the case passed validation)] of `lib` (a loaded _lib), in the order of cases()"""
    from myldpccppapi_amd import _lib
    out = []
    for name, fields in cases():
        cfg = _lib.DecoderConfigBf()
        assert lib.ldpc_decoder_config_init_sized(ctypes.byref(cfg), ctypes.sizeof(cfg)) == 0
        cfg.K, cfg.max_batch, cfg.layer_rows, cfg.device = K, 64, Z, NO_DEVICE
        for k, v in fields.items():
            if k == "bf_threshold0":
                cfg.bf_threshold[0] = v
            else:
                setattr(cfg, k, v)
        h = ctypes.c_void_p()
        rc = lib.ldpc_decoder_create(g._h, ctypes.byref(cfg), ctypes.byref(h))
        assert rc != 0 and not h.value, name        # no machine has that device
        msg = lib.ldpc_last_error().decode()
        out.append((rc, None if rc == LDPC_ERR_HIP else msg))   # no validation refusal carries LDPC_ERR_HIP
    return out


if __name__ == "__main__":
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["LDPC_HIP_LIB"] = sys.argv[1]
    from myldpccppapi_amd import _lib
    got = answers(_lib.load(), graph())
    messages = sorted({m for _, m in got if m is not None})
    where = {m: i for i, m in enumerate(messages)}
    np.savez_compressed(sys.argv[2], messages=np.array(messages), code=np.array([c for c, _ in got], np.int8),
                        index=np.array([-1 if m is None else where[m] for _, m in got], np.int16),
                        names_sha256=np.array(names_sha256()))
    print("%d cases, %d distinct messages, %d passed validation" % (len(got), len(messages), sum(m is None for _, m in got)))

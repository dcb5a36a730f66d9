"""The expectation of CRC-aided early termination (include/ldpc_hip.h: crc_kind / crc_bits), from the CPU oracle (or
another restatement that freezes on the syndrome) and tb_ref alone -- never from the library under test.

A reference that freezes frames on a clean syndrome, run with max_iter = i, leaves the hard bits b_i of every frame that
was still running when round i began.  crc_rule() runs it for i = 1 .. max_iter on the frames that are still running,
tests every frame for clean_i (the syndrome of b_i) and crc_i (tb_ref's long division over b_i[:crc_bits]) and freezes it
at the first round where either holds.  Frames freeze independently, so handing only the running frames on changes
nothing about them."""
import numpy as np

import oracle
import tb_ref
from util import converged_frames


def oracle_decoder(g, algo, llr_scale=8.0, layer_rows=0, msg_f16=False):
    """decode(y, i) -> hard uint8 [frames, N] of oracle.decode with max_iter = i."""
    def decode(y, i):
        return oracle.decode(g, y, algo, max_iter=i, llr_scale=llr_scale, layer_rows=layer_rows, msg_f16=msg_f16)["hard"]
    return decode


def crc_passes(kind, bits):
    """bool [frames]: the rows leave remainder zero."""
    bits = np.asarray(bits, np.uint8)
    if bits.shape[0] == 0:
        return np.zeros(0, bool)
    return ~tb_ref.parity(kind, bits).any(axis=1)


def crc_rule(decode, y, rows, cols, M, N, K, kind, bits, max_iter):
    """dict(out = bytes as LDPC_PACK_BYTES packs them, iters int32 [frames], hard uint8 [frames, N],
            by_crc = frames frozen in a round in which their syndrome was not clean (what ldpc_decoder_crc_stops counts),
            syn_iters / syn_clean = round and success of the syndrome rule alone,
            earlier = frames the CRC stops before the syndrome would (or where it never would),
            crc_only = those of them the syndrome never stops, never = frames neither rule stops)."""
    assert K % 8 == 0
    y = np.ascontiguousarray(y, np.float32).reshape(-1, N)
    frames = y.shape[0]
    hard = np.zeros((frames, N), np.uint8)
    iters = np.full(frames, max_iter, np.int32)
    frozen = np.zeros(frames, bool)
    by_crc = np.zeros(frames, bool)
    syn_iters = np.full(frames, max_iter, np.int32)
    syn_clean = np.zeros(frames, bool)
    A = np.arange(frames)                         # running under the combined rule
    S = np.ones(frames, bool)                     # running under the syndrome rule alone (a superset of A's frames)
    for i in range(1, max_iter + 1):
        # the syndrome rule alone needs the frames the CRC has already stopped as well
        idx = np.nonzero(S)[0]
        if idx.size == 0:
            break
        h = decode(y[idx], i)
        clean = converged_frames(rows, cols, M, h)
        syn_iters[idx[clean]] = i
        syn_clean[idx[clean]] = True
        S[idx[clean]] = False
        pos = np.searchsorted(idx, A)             # A is a subset of idx
        hA, cleanA = h[pos], clean[pos]
        crcA = crc_passes(kind, hA[:, :bits])
        hard[A] = hA
        stop = cleanA | crcA
        iters[A[stop]] = i
        frozen[A[stop]] = True
        by_crc[A[stop & ~cleanA]] = True
        A = A[~stop]
    earlier = np.nonzero(frozen & (~syn_clean | (iters < syn_iters)))[0]
    assert np.array_equal(earlier, np.nonzero(by_crc)[0])
    return dict(out=np.packbits(hard[:, :K], axis=1, bitorder="little").reshape(-1), iters=iters, hard=hard,
                by_crc=np.nonzero(by_crc)[0], syn_iters=syn_iters, syn_clean=syn_clean, earlier=earlier,
                crc_only=np.nonzero(frozen & ~syn_clean)[0], never=np.nonzero(~frozen)[0])


# ---- the chain scenario of tb_util (BG1-profile code, Z = 16, CRC16 over Kp = 328 bits, 64 frames, 20 rounds) -------------
import functools

CHAIN_KIND, CHAIN_BITS = 16, 328


@functools.lru_cache(maxsize=None)
def chain(algo, snr_db, variant=""):
    """crc_rule() on the chain scenario; variant "" | "f16" (fp16 messages, the oracle's msg_f16) | "scale" (ms_scale =
    0.75, tests/ms_correction_ref.py).  Computed once per process, read-only."""
    import ratematch_util as U
    import tb_util as TU
    rows, cols, g = U.bg1()
    y = TU.chain_received(snr_db)[2]
    if variant == "scale":
        from ms_correction_ref import Code, flood_ms
        code = Code(rows, cols, U.M, U.N, U.K)
        decode = lambda ys, i: flood_ms(code, ys, i, scale=0.75)["hard"]        # noqa: E731
    else:
        decode = oracle_decoder(g, algo, llr_scale=TU.HARD[algo][1], layer_rows=U.Z, msg_f16=variant == "f16")
    r = crc_rule(decode, y, rows, cols, U.M, U.N, U.K, CHAIN_KIND, CHAIN_BITS, U.MAX_ITER)
    for v in r.values():
        v.setflags(write=False)
    return r

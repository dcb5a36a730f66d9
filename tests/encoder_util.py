"""Helpers of the encoder tests: the expected bytes (oracle.gf2_encoder, never the code under test), the syndrome and
information part of encoded frames in numpy, and the build of tests/cpp/coder_device_encode.cpp."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def frame_starts(K, frames):
    """Byte at which frame f reads its source: (f*K)/8, the product first (Coder::encode)."""
    return [(f * K) // 8 for f in range(frames)]


def stream_length(K, frames, cut=0):
    """Bytes of a source stream of `frames` frames whose last frame lacks `cut` bytes."""
    return (frames - 1) * K // 8 + K // 8 - cut


def reference_packed(ge, src, frames):
    """uint8 [frames, N/8]: oracle.gf2_encoder.Gf2Encoder.encode_bytes frame by frame on the source stream `src`."""
    kb = ge.K // 8
    out = np.zeros((frames, ge.N // 8), np.uint8)
    for f, at in enumerate(frame_starts(ge.K, frames)):
        out[f] = ge.encode_bytes(src[at:at + kb].tobytes())
    return out


def info_bits(K, src, frames):
    """uint8 [frames, K]: the information bits the conventions prescribe (whole bytes only, short tail zero)."""
    kb = K // 8
    bits = np.zeros((frames, K), np.uint8)
    for f, at in enumerate(frame_starts(K, frames)):
        chunk = src[at:at + kb]
        bits[f, :chunk.size * 8] = np.unpackbits(chunk, bitorder="little")
    return bits


def syndrome_weight(rows, cols, M, bits):
    """Number of unsatisfied checks over all frames; bits uint8 [frames, N]; rows/cols row-major (every row has an edge)."""
    rows = np.asarray(rows)
    ptr = np.searchsorted(rows, np.arange(M))
    total = 0
    for lo in range(0, bits.shape[0], 32):
        per_edge = np.ascontiguousarray(bits[lo:lo + 32].T)[np.asarray(cols)]        # [E, frames]
        total += int(np.bitwise_xor.reduceat(per_edge, ptr, axis=0).sum())
    return total


def coder_device_encode_exe(tmp_path):
    exe = str(tmp_path / "coder_device_encode")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "coder_device_encode.cpp"), "-o", exe,
                           "-L" + os.path.join(ROOT, "myldpccppapi_amd"), "-lmyldpc", "-lldpc_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myldpccppapi_amd")])
    return exe

/*
 * row_io.hpp -- how a lane of the row-walking kernels (tb_kernels.hpp, bch_kernels.hpp) takes the bytes of its run out of
 * a row and puts bytes into one, 16 at a time where address and length allow, and the XOR reduction over a wave.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ldpc {

/* bytes p[i], p[i + 1], ... one at a time; bytes from `lim` on read as zero.  The buffer is refilled with one 16-byte
 * load where the address allows and all 16 bytes lie in front of `lim`; otherwise with the bytes up to the next 16-byte
 * boundary (or up to `lim`), loaded independently of one another, so that a run costs one memory latency for its
 * unaligned head, one per 16 bytes, and one for its tail */
struct TbSource {
    const uint8_t *p;
    int64_t i, lim;
    uint64_t lo = 0, hi = 0;
    int have = 0;
    __device__ TbSource(const uint8_t *p_, int64_t i_, int64_t lim_) : p(p_), i(i_), lim(lim_) {}
    __device__ void refill()
    {
        lo = hi = 0;
        have = 16;
        if (i >= lim) return;                                   /* zeros from here on */
        const int to_boundary = 16 - (int)(reinterpret_cast<uintptr_t>(p + i) & 15);
        if (to_boundary == 16 && i + 16 <= lim) {
            const uint4 q = *reinterpret_cast<const uint4 *>(p + i);
            lo = (uint64_t)q.x | ((uint64_t)q.y << 32);
            hi = (uint64_t)q.z | ((uint64_t)q.w << 32);
            return;
        }
        have = (int)min((int64_t)to_boundary, lim - i);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint64_t b = k < have ? p[i + k] : 0;
            if (k < 8) lo |= b << (8 * k);
            else hi |= b << (8 * (k - 8));
        }
    }
    __device__ uint32_t next()
    {
        if (have == 0) refill();
        const uint32_t b = (uint32_t)lo & 0xffu;
        lo = (lo >> 8) | (hi << 56);
        hi >>= 8;
        --have;
        ++i;
        return b;
    }
};

/* exactly end - i bytes are pushed; 16-byte stores where the address allows and 16 more bytes are to come */
struct TbSink {
    uint8_t *p;
    int64_t i, end;
    uint64_t lo = 0, hi = 0;
    int n = 0;
    __device__ TbSink(uint8_t *p_, int64_t i_, int64_t end_) : p(p_), i(i_), end(end_) {}
    __device__ void push(uint32_t b)
    {
        if (n == 0 && !(i + 16 <= end && (reinterpret_cast<uintptr_t>(p + i) & 15) == 0)) {
            p[i++] = (uint8_t)b;
            return;
        }
        if (n < 8) lo |= (uint64_t)b << (8 * n);
        else hi |= (uint64_t)b << (8 * (n - 8));
        if (++n == 16) {
            *reinterpret_cast<uint4 *>(p + i) = uint4{(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
            i += 16;
            n = 0;
            lo = hi = 0;
        }
    }
};

__device__ inline uint32_t tb_wave_xor(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v ^= __shfl_xor(v, o);
    return v;
}

}  // namespace ldpc

/*
 * ldsp_fx_kernels.hpp -- LDPC_ALGO_LAYERED_FX (fixed-point layered min-sum, include/ldpc_hip.h has the rule bit for bit) on
 * the record organisation of ldsp_kernels.hpp: layered_ldsp_kernel's placement, schedule and frame with the integer row.
 * Selected by LDPC_TUNE_ON(LDPC_TUNE_FX_RECORD) only; the results are those of the streaming engine (kLayerFx) bit for bit.
 *
 * Data placement, per frame (one persistent workgroup = one frame at a time, lanes = the z rows of a layer):
 *   - posteriors of the block columns met by two or more layers: int16_t P[lds_cols][z] from LDS address 0 (BG1 Z = 384:
 *     20 KB), the workgroup flag word behind it at the next 4-byte boundary;
 *   - a block column met by one layer only travels with that row's record;
 *   - the row's state is the 8-byte record, read and written by the row's own lane only:
 *         x = signs of R_0 .. R_{D-1} in bits 0 .. 23 | argmin << 24
 *         y = m1' | m2' << 8 | (int16 posterior of the row's single-layer column) << 16
 *     m1', m2': the two candidates after the correction and the clamp to L (<= 127).  The old message is
 *     R_k = (sign_k ? -1 : 1) * (k == argmin ? m2' : m1').  A magnitude of 0 makes the sign immaterial (-0 = 0 in integers),
 *     so there is no zero flag and no slow path; NaN does not exist.  Where several entries tie for the minimum, m1 = m2 and
 *     every argmin among them rebuilds the same messages: the kernel keeps the first, as the definition does, and nothing
 *     depends on it.
 * The rings hold layers * z records per resident workgroup plus a spare tail: every lane of the block requests the next
 * record, lanes beyond the last row included (never used).
 * Arithmetic: t_k = P - R_old in 32 bits; the row reads clamp(t_k, -L, L); two smallest magnitudes; the correction in fp32,
 * once per row, on the two candidates (plain min-sum is scale 1 / offset 0, the identity on [0, L], as on the streaming
 * engine); P_new = clamp(t_k + R_k, -LP, LP) from the unclamped t_k, stored as int16.  The clamp to L is taken on the two
 * minima instead of on every entry: clamping is monotone, so the two smallest of the clamped magnitudes are the clamped two
 * smallest, and the argmin can differ only where both read L.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "layered_kernels.hpp"
#include "ldsp_kernels.hpp"

namespace ldpc {

constexpr int kFxStart = 1000;          /* the start value of the two minima: the candidate of a row of degree 1 */

struct LdspFxArgs {
    const float *__restrict__ llr;        /* [frames][N] */
    uint8_t *__restrict__ out;            /* packed bytes, toChar layout */
    int32_t *__restrict__ iters;          /* [frames] or nullptr */
    int32_t *__restrict__ summary;        /* [2]: max iters, converged frames */
    float *__restrict__ dump_p;           /* [frames][N] or nullptr (taps, soft output) */
    float *__restrict__ dump_r;           /* [frames][E] reference edge order, or nullptr */
    uint2 *__restrict__ recs;             /* [grid][layers*z] check records + spare tail */
    const int32_t *__restrict__ hdr;      /* [layers][4]: as LdspArgs::hdr */
    const int32_t *__restrict__ pack;     /* [layers][4][24]: as LdspArgs::pack, in units of 2 bytes */
    const int32_t *__restrict__ col_slot; /* [N/z] */
    const int32_t *__restrict__ layer_e0; /* [layers] */
    int64_t frames, out_bytes;
    int32_t N, E, K, z, layers, nb, lds_cols, max_iter, rounds, early_term;
    int32_t L, LP;                        /* 2^(q-1) - 1, 2^(p-1) - 1 */
    float llr_scale;                      /* LSBs per unit of channel value */
    MsCorr corr;                          /* scale (1 = none), offset */
};

typedef __attribute__((address_space(3))) int16_t ldpc_lds_i16;

/* ldsp_at_abs with two-byte cells: r2 = 2r, colshift = 2 (slot z + shift), thresh = 2 (z - shift), negz2 = -2z */
__device__ __forceinline__ ldpc_lds_i16 *ldsp_fx_at(int colshift, int thresh, int r2, int negz2)
{
    const uint32_t wrap = (uint32_t)r2 >= (uint32_t)thresh ? (uint32_t)negz2 : 0u;
    uint32_t at;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(at) : "v"(r2), "s"(colshift), "v"(wrap));
    return reinterpret_cast<ldpc_lds_i16 *>((uintptr_t)at);
}

__device__ __forceinline__ int fx_med3(int a, int lo, int hi) { return min(max(a, lo), hi); }

/* the record's words from their fields, and message k of a record */
__device__ __forceinline__ uint2 ldsp_fx_pack(uint32_t signs, int argmin, int m1, int m2, int ext)
{
    return uint2{signs | ((uint32_t)argmin << 24), (uint32_t)m1 | ((uint32_t)m2 << 8) | ((uint32_t)ext << 16)};
}
__device__ __forceinline__ int ldsp_fx_ext(const uint2 rec) { return (int)rec.y >> 16; }
__device__ __forceinline__ int ldsp_fx_message(const uint2 rec, int k)
{
    const int mag = (int)((k == (int)((rec.x >> 24) & 31u) ? rec.y >> 8 : rec.y) & 255u);
    return ((rec.x >> k) & 1u) ? -mag : mag;
}

/* Exact row width (DL entries in LDS + EXT external), straight-line code, any input. */
template <int DL, int EXT>
__device__ __forceinline__ uint2 ldsp_fx_row(ldpc_const_i32 pk, int z, int r, const uint2 old, int L, int LP, const MsCorr corr)
{
    constexpr int D = DL + EXT;
    constexpr int DLA = DL > 0 ? DL : 1;
    ldpc_lds_i16 *at[DLA];
#pragma unroll
    for (int k = 0; k < DL; ++k) at[k] = ldsp_fx_at(pk[2 * kLdspMaxDeg + k], pk[3 * kLdspMaxDeg + k], r * 2, -(z * 2));
    int t[D];
#pragma unroll
    for (int k = 0; k < D; ++k) t[k] = (k < DL ? (int)*at[k < DL ? k : 0] : ldsp_fx_ext(old)) - ldsp_fx_message(old, k);
    /* the hard decisions x_k < 0 = t_k < 0 (L > 0) as a mask, bit k; their parity is the row's sign */
    uint32_t neg = 0;
#pragma unroll
    for (int k = D - 1; k >= 0; --k) neg = __builtin_amdgcn_alignbit(neg, (uint32_t)t[k], 31);     /* (neg << 1) | sign(t_k) */
    int m1 = kFxStart, m2 = kFxStart, idx = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const int mag = max(t[k], -t[k]);
        idx = mag < m1 ? k : idx;                                   /* the first smallest */
        m2 = fx_med3(mag, m1, m2);                                  /* m1 <= m2: m1 if below both, m2 if above both */
        m1 = min(m1, mag);
    }
    m1 = min(m1, L);                                                /* D >= 1: |x| <= L */
    if (D > 1) m2 = min(m2, L);                                     /* D = 1: the start value itself is the candidate */
    const float Lf = (float)L;
    m1 = (int)fx_corr((float)m1, corr, Lf);                         /* once per row */
    m2 = (int)fx_corr((float)m2, corr, Lf);
    const uint32_t signs = (__builtin_popcount(neg) & 1) ? (neg ^ ((1u << D) - 1u)) : neg;         /* par ^ neg_k */
    int pext = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const int b = (k == idx) ? m2 : m1;
        const int rn = ((signs >> k) & 1u) ? -b : b;
        const int pn = fx_med3(t[k] + rn, -LP, LP);                 /* from the unclamped t_k */
        if (k < DL) *at[k < DL ? k : 0] = (int16_t)pn;
        else pext = pn;
    }
    return ldsp_fx_pack(signs, idx, m1, m2, pext & 0xffff);
}

/* parities of the hard decisions P < 0 over the LDS entries of the wave's rows, as a lane mask */
template <int DL>
__device__ __forceinline__ uint64_t ldsp_fx_row_parity(ldpc_const_i32 pk, int z, int r)
{
    int v[DL];
#pragma unroll
    for (int k = 0; k < DL; ++k) v[k] = *ldsp_fx_at(pk[2 * kLdspMaxDeg + k], pk[3 * kLdspMaxDeg + k], r * 2, -(z * 2));
    uint64_t par = 0;
#pragma unroll
    for (int k = 0; k < DL; ++k) par ^= __ballot(v[k] < 0);
    return par;
}

/* tap / soft output: the frame's posteriors as floats, the LDS-resident columns from P and the others from their records */
__device__ __forceinline__ void ldsp_fx_dump_p(const LdspFxArgs &a, const int16_t *P, const uint2 *recs, int64_t frame, int r)
{
    const ldpc_const_i32 hdr = as_constant(a.hdr), cslot = as_constant(a.col_slot);
    const int z = a.z;
    for (int bc = 0; bc < a.nb; ++bc) {
        const int slot = cslot[bc];
        if (slot >= 0) a.dump_p[(size_t)frame * a.N + bc * z + r] = (float)P[slot * z + r];
    }
    for (int l = 0; l < a.layers; ++l)
        if (hdr[l * 4 + 1])
            a.dump_p[(size_t)frame * a.N + hdr[l * 4 + 2] + ldsp_wrap(r, hdr[l * 4 + 3], z)] = (float)ldsp_fx_ext(recs[(size_t)l * z]);
}

/* tap: the frame's check-to-variable messages in the reference's edge order, rebuilt from the records */
__device__ __forceinline__ void ldsp_fx_dump_r(const LdspFxArgs &a, const uint2 *recs, int64_t frame, int r)
{
    const ldpc_const_i32 hdr = as_constant(a.hdr);
    const int z = a.z;
    for (int l = 0; l < a.layers; ++l) {
        const int d = hdr[l * 4] + hdr[l * 4 + 1], e0 = a.layer_e0[l];
        const uint2 rec = recs[(size_t)l * z];
        for (int k = 0; k < d; ++k) a.dump_r[(size_t)frame * a.E + e0 + r * d + k] = (float)ldsp_fx_message(rec, k);
    }
}

template <int MAXW>
__global__ __launch_bounds__(64 * MAXW) __attribute__((amdgpu_waves_per_eu(LDPC_LDSP_WAVES_PER_EU)))
void layered_ldsp_fx_kernel(const LdspFxArgs a)
{
    extern __shared__ int16_t lds_fx[];
    int16_t *P = lds_fx;                                                        /* [lds_cols][z], LDS address 0 */
    const int r = (int)threadIdx.x, LANES = (int)blockDim.x;
    const int z = a.z;
    uint32_t *wg_flag = reinterpret_cast<uint32_t *>(lds_fx + (((size_t)a.lds_cols * z + 1) & ~(size_t)1));
    const bool row = r < z;
    uint2 *recs = a.recs + (size_t)blockIdx.x * ((size_t)a.layers * z) + r;     /* [layer][z], mine: + r */
    const ldpc_const_i32 hdr = as_constant(a.hdr), pack = as_constant(a.pack), cslot = as_constant(a.col_slot);
    const int L = a.L, LP = a.LP;
    const float Lf = (float)L;
    const MsCorr corr = a.corr;
    for (int64_t frame = blockIdx.x; frame < a.frames; frame += gridDim.x) {
        const float *y = a.llr + (size_t)frame * a.N;
        if (row) {
            for (int bc = 0; bc < a.nb; ++bc) {
                const int slot = cslot[bc];
                if (slot >= 0) P[slot * z + r] = (int16_t)(int)layer_chan<StoreFx, false>(y[bc * z + r], a.llr_scale, Lf);
            }
            /* round 0: R = 0 (m1' = m2' = 0); an external column starts from its channel value */
            for (int l = 0; l < a.layers; ++l) {
                int c = 0;
                if (hdr[l * 4 + 1])
                    c = (int)layer_chan<StoreFx, false>(y[hdr[l * 4 + 2] + ldsp_wrap(r, hdr[l * 4 + 3], z)], a.llr_scale, Lf);
                recs[(size_t)l * z] = ldsp_fx_pack(0u, 0, 0, 0, c & 0xffff);
            }
        }
        uint2 cur = uint2{0u, 0u};
        if (row) cur = recs[0];
        __syncthreads();
        int time = 0;
        bool clean = false;
        /* lane mask of the wave's rows of layer l whose hard decisions have odd parity */
        auto layer_odd = [&](const int l) {
            const int dl = hdr[l * 4], ext = hdr[l * 4 + 1];
            const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
            uint64_t par = 0;
            switch (dl) {
#define LDPC_LDSP_CASE(D) case D + 1: par = ldsp_fx_row_parity<D + 1>(pk, z, r); break;
                LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
            default: break;
            }
            if (ext) par ^= __ballot(ldsp_fx_ext(recs[(size_t)l * z]) < 0);     /* its posterior is in my record */
            return par;
        };
        while (true) {
            for (int l = 0; l < a.layers; ++l) {
                /* the next layer step's record, requested before this step's work by every lane, outside any branch (see
                 * layered_ldsp_kernel); lanes beyond the last row read inside the ring or its spare tail */
                const int ln = l + 1 < a.layers ? l + 1 : 0;
                uint2 nxt = recs[(size_t)ln * z];
                const int dl = hdr[l * 4], ext = hdr[l * 4 + 1];
                const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                uint2 rec = uint2{0u, 0u};
                if (row) {
                    if (ext) {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D: rec = ldsp_fx_row<D, 1>(pk, z, r, cur, L, LP, corr); break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    } else {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D + 1: rec = ldsp_fx_row<D + 1, 0>(pk, z, r, cur, L, LP, corr); break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    }
                }
                /* take the requested record before the store below is issued (see layered_ldsp_kernel) */
                asm volatile("" : "+v"(nxt.x), "+v"(nxt.y) : : "memory");
                if (row) recs[(size_t)l * z] = rec;
                if (a.layers == 1) nxt = rec;
                lds_barrier();
                cur = nxt;
            }
            /* syndrome of the hard decisions: every round when a clean frame stops early, else after the last one only */
            ++time;
            int any_bad = 1;
            if (a.early_term || time == a.rounds) {
                uint64_t bad = row ? layer_odd(a.layers - 1) : 0ull;
                if (!ldsp_wg_any(wg_flag, r, bad != 0ull)) {
                    if (row)
                        for (int l = 0; l + 1 < a.layers; ++l) bad |= layer_odd(l);
                    any_bad = ldsp_wg_any(wg_flag, r, bad != 0ull) ? 1 : 0;
                }
            }
            clean = !any_bad;
            if ((clean && a.early_term) || time == a.rounds) break;
        }
        /* toChar: the information columns sit in LDS at slot = block column */
        const int64_t base = frame * (int64_t)a.K / 8;
        for (int j = r; j < a.K / 8; j += LANES) {
            unsigned byte = 0;
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) byte |= (P[j * 8 + bit] < 0 ? 1u : 0u) << bit;
            if (base + j < a.out_bytes) a.out[base + j] = (uint8_t)byte;
        }
        if (a.dump_p && row) ldsp_fx_dump_p(a, P, recs, frame, r);
        if (a.dump_r && row) ldsp_fx_dump_r(a, recs, frame, r);
        if (r == 0) ldsp_report(a, frame, clean ? time : a.max_iter, clean);
        __syncthreads();                                           /* P is refilled for the next frame */
    }
}

/* compiled by engine_ldsp_fx.hip only (LDPC_ENGINE_LDSP_FX); the host driver calls engine_ldsp_fx_plan_create /
 * engine_ldsp_fx_run */
#ifdef LDPC_ENGINE_LDSP_FX

/* The plan of layered_ldsp_fx_kernel: ldsp_plan_layout with two-byte cells and no packed form, 8-byte records.  Before
 * the call: pl->mc (scale 1 = none), pl->fx_L, pl->fx_LP.  eligible = false (and hipSuccess) when the code does not fit. */
inline hipError_t ldsp_fx_plan_create(LdspPlan *pl, int32_t M, int32_t N, int64_t E, const std::vector<int32_t> &row_ptr,
                                      const std::vector<int32_t> &cols, int32_t z, int32_t K, int64_t max_batch, int device,
                                      const Tune &tune)
{
    hipError_t e;
    pl->fx = 1;
    if ((e = ldsp_plan_layout(pl, M, N, E, row_ptr, cols, z, K, tune, /*flood=*/0, /*cell=*/sizeof(int16_t)))) return e;
    if (!pl->laid_out) return hipSuccess;
    pl->kernel = pl->maxw <= 8 ? (const void *)layered_ldsp_fx_kernel<8> : (const void *)layered_ldsp_fx_kernel<16>;
    /* Workgroups of 5 .. 7 waves: at most 3 per CU.  Measured at BG1 Z = 384 (6 waves, 8192 frames, 20 rounds, two alternating
     * windows, profiles/layered_fx_record.txt): 3 per CU 21.13 / 21.11 ms, the 4 that registers, LDS and the cache rule allow
     * 21.66 / 21.68 ms, 2 per CU 24.5 ms; at Z = 64, 128 and 256 (1, 2, 4 waves) the unbounded choice is the best of the sweep.
     * Why: a supposition only -- the dispatcher places such a workgroup's waves 2-2-1-1 on the four SIMDs (ldsp_kernels.hpp),
     * so a fourth one fills every SIMD to the budget of LDPC_LDSP_WAVES_PER_EU and the barrier of each layer step waits for
     * the most crowded SIMD.  The bound is the budget over a workgroup's waves on its busiest SIMD. */
    const int waves = pl->block / 64;
    const int cap = (waves > 4 && waves % 4) ? LDPC_LDSP_WAVES_PER_EU / ((waves + 3) / 4) : 0;
    if ((e = ldsp_plan_grid(pl, max_batch, device, tune, sizeof(uint2), cap))) return e;
    /* + 1024 (the largest workgroup): lanes beyond the last row request records too (never used) */
    if ((e = pl->recs_fx.alloc((size_t)pl->grid * M + 1024))) return e;
    pl->eligible = true;
    return hipSuccess;
}

/* one persistent grid for the whole batch */
inline hipError_t ldsp_fx_run(LdspPlan *pl, const FusedRun &r, hipStream_t s, int32_t *launched)
{
    hipError_t e;
    if ((e = hipMemsetAsync(r.summary, 0, 2 * sizeof(int32_t), s))) return e;
    const int rounds = r.tap_iter ? (r.tap_iter < r.max_iter ? r.tap_iter : r.max_iter) : r.max_iter;
    if (r.tap_iter && pl->dump_frames < r.frames) {
        if ((e = pl->dump_p.alloc((size_t)r.frames * pl->N))) return e;
        if ((e = pl->dump_r.alloc((size_t)r.frames * pl->E))) return e;
        pl->dump_frames = r.frames;
    }
    LdspFxArgs a{r.llr_dev, r.out_dev, r.iters_dev, r.summary, r.soft ? r.soft : (r.tap_iter ? pl->dump_p.p : nullptr),
                 r.tap_iter ? pl->dump_r.p : nullptr, pl->recs_fx.p, pl->hdr.p, pl->pack.p, pl->col_slot.p, pl->layer_e0.p,
                 r.frames, r.out_dev ? r.out_bytes : 0, pl->N, pl->E, r.K, pl->z, pl->layers, pl->nb, pl->lds_cols,
                 r.max_iter, rounds, r.early_term, pl->fx_L, pl->fx_LP, r.llr_scale, pl->mc};
    const unsigned grid = (unsigned)std::min<int64_t>(r.frames, pl->grid);
    if (!pl->eligible || !pl->fx || grid == 0) return hipErrorInvalidValue;
    void *args[1] = {&a};
    if ((e = hipLaunchKernel(pl->kernel, dim3(grid), dim3((unsigned)pl->block), args, pl->lds_bytes, s))) return e;
    *launched = rounds;
    if ((e = hipGetLastError())) return e;
    /* soft output, extrinsic kind: P - c with c = sq(llr_scale * y), the streaming engine's pass (not P - y) */
    if (r.soft && r.soft_extrinsic) {
        const int64_t count = r.frames * (int64_t)pl->N;
        layered_extrinsic_kernel<float, StoreFx><<<(unsigned)((count + kBlock - 1) / kBlock), kBlock, 0, s>>>(
            r.soft, r.llr_dev, r.llr_scale, (float)pl->fx_L, count, 1.0f);
        return hipGetLastError();
    }
    return hipSuccess;
}

#endif  /* LDPC_ENGINE_LDSP_FX */

}  // namespace ldpc

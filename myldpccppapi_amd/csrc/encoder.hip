/*
 * encoder.hip -- the "encoder" section of the C ABI (include/ldpc_hip.h): host analysis of the parity part of H,
 * the encoder handle, and the launches of encoder_kernels.hpp.  Data conventions are those of Coder::encode /
 * encodeOnce (MyLdpc.cpp), so that the bytes equal the host encoder's.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/ldpc_hip.h"
#include "encoder_dense.hpp"
#include "encoder_kernels.hpp"
#include "graph.hpp"
#include "hip_host.hpp"

using ldpc::set_error;
using ldpc::DevBuf;

namespace {

struct ParityStructure {
    int32_t kind = 0, c = 0, x = 0, a = 0, b = 0, ext = 0, z = 0;
};

/* parity column K + m has its ones in rows m and m + 1 only (the last one: row M - 1 only) */
bool is_staircase(const ldpc_graph *g, int32_t K)
{
    const int32_t M = g->M;
    for (int32_t m = 0; m < M; ++m) {
        const int32_t p0 = g->col_ptr[K + m], p1 = g->col_ptr[K + m + 1];
        if (p1 - p0 != (m + 1 < M ? 2 : 1)) return false;
        if (g->rows[g->col_edge[p0]] != m) return false;                    /* a column's edges ascend by row */
        if (m + 1 < M && g->rows[g->col_edge[p0 + 1]] != m + 1) return false;
    }
    return true;
}

int analyse(const ldpc_graph *g, int32_t K, int32_t z, ParityStructure *ps)
{
    if (!g) return set_error(LDPC_ERR_ARG, "graph is NULL");
    if (K <= 0 || K >= g->N || g->N - K != g->M)
        return set_error(LDPC_ERR_ARG, "K = %d does not match the graph: systematic encoding needs K = N - M = %d", K, g->N - g->M);
    if (z < 0) return set_error(LDPC_ERR_ARG, "block_rows = %d is negative", z);
    *ps = ParityStructure();
    if (is_staircase(g, K)) {
        ps->kind = LDPC_PARITY_STAIRCASE;
        return LDPC_OK;
    }
    if (z == 0)
        return set_error(LDPC_ERR_UNSUPPORTED, "parity part is not a staircase and block_rows = 0 names no circulant size");
    if (g->M % z || K % z)
        return set_error(LDPC_ERR_UNSUPPORTED, "block_rows = %d does not divide M = %d and K = %d", z, g->M, K);
    const int32_t mb = g->M / z;
    /* every block of the parity part is empty or one circulant permutation: z edges of one shift */
    std::vector<int32_t> cnt((size_t)mb * mb, 0), sh((size_t)mb * mb, -1);
    for (int64_t e = 0; e < g->E; ++e) {
        if (g->cols[e] < K) continue;
        const int32_t r = g->rows[e], q = g->cols[e] - K;
        const int32_t i = r / z, j = q / z, p = ((q % z) - (r % z) + z) % z;
        const size_t at = (size_t)i * mb + j;
        if (cnt[at] == 0) sh[at] = p;
        else if (sh[at] != p)
            return set_error(LDPC_ERR_UNSUPPORTED, "parity block (%d, %d) is not a circulant of %d rows (shifts %d and %d)", i, j, z, sh[at], p);
        ++cnt[at];
    }
    for (size_t at = 0; at < cnt.size(); ++at)
        if (cnt[at] && cnt[at] != z)
            return set_error(LDPC_ERR_UNSUPPORTED, "parity block (%d, %d) has %d of the %d ones of a circulant", (int)(at / mb), (int)(at % mb), cnt[at], z);
    auto has = [&](int32_t i, int32_t j) { return cnt[(size_t)i * mb + j] != 0; };
    auto shift = [&](int32_t i, int32_t j) { return sh[(size_t)i * mb + j]; };
    /* extension: the trailing parity block columns whose only block is a zero-shift identity in their own block row */
    int32_t c = mb;
    while (c > 0) {
        const int32_t j = c - 1;
        int32_t blocks = 0;
        for (int32_t i = 0; i < mb; ++i) blocks += has(i, j);
        if (blocks == 1 && has(j, j) && shift(j, j) == 0) --c; else break;
    }
    if (c < 3) return set_error(LDPC_ERR_UNSUPPORTED, "parity part has no dual-diagonal core (%d core block rows)", c);
    /* core rows touch core parity columns only (the extension columns are single blocks in extension rows); the first
     * core column has three blocks in core rows 0, x, c-1 with shifts (a, b, a) */
    int32_t three[3], n3 = 0;
    for (int32_t i = 0; i < c; ++i)
        if (has(i, 0)) { if (n3 < 3) three[n3] = i; ++n3; }
    if (n3 != 3 || three[0] != 0 || three[2] != c - 1)
        return set_error(LDPC_ERR_UNSUPPORTED, "first parity block column has %d blocks in the %d core block rows; wanted 3, in rows 0, x and %d", n3, c, c - 1);
    if (shift(0, 0) != shift(c - 1, 0))
        return set_error(LDPC_ERR_UNSUPPORTED, "first parity block column: outer shifts %d and %d differ", shift(0, 0), shift(c - 1, 0));
    for (int32_t j = 1; j < c; ++j)
        for (int32_t i = 0; i < c; ++i) {
            const bool want = (i == j - 1 || i == j);
            if (want ? (!has(i, j) || shift(i, j) != 0) : has(i, j))
                return set_error(LDPC_ERR_UNSUPPORTED, "parity block column %d is not on the zero-shift dual diagonal (block row %d)", j, i);
        }
    ps->kind = LDPC_PARITY_DUAL_DIAGONAL;
    ps->c = c; ps->x = three[1]; ps->a = shift(0, 0); ps->b = shift(three[1], 0); ps->ext = mb - c; ps->z = z;
    return LDPC_OK;
}

}  // namespace

struct ldpc_encoder {
    int32_t device = 0, N = 0, K = 0, M = 0, max_frames = 0, Wmax = 0, chunks = 0;
    ParityStructure ps;
    DevBuf<uint64_t> X;        /* [N][W] bit-sliced codewords                                        */
    DevBuf<uint64_t> aux;      /* dual diagonal: lambda of the core rows [c z][W]; staircase: chunk totals;
                                  dense: lambda of all rows [M][W]                                      */
    DevBuf<uint64_t> T;        /* dense: the solve matrix [N - K][tw]                                   */
    int32_t tw = 0;
    DevBuf<int32_t> ptr, col;  /* per row: the columns lambda_m (or an extension row's parity bit) sums  */
    DevBuf<uint8_t> src_stage, code_stage;   /* ldpc_encode(): made on its first call               */
};

namespace {

/* frames [first, first + frames) of the caller's stream; src_dev points at byte (first K) / 8 of it */
int enqueue(ldpc_encoder *e, const uint8_t *src_dev, int64_t src_bytes, int64_t first, int64_t frames, uint8_t *code_dev,
            int32_t format, hipStream_t s)
{
    using namespace ldpc;
    const int32_t W = (int32_t)((frames + 63) / 64);
    const unsigned wt = (unsigned)((W + 63) / 64);
    auto blocks = [](int64_t n) { return (unsigned)((n + kEncWaves - 1) / kEncWaves); };
    uint64_t *X = e->X.p, *P = e->X.p + (size_t)e->K * W;
    enc_load_kernel<<<dim3(blocks((e->K + 63) / 64), (unsigned)W), kEncBlock, 0, s>>>(src_dev, src_bytes, first, first * (int64_t)e->K / 8,
                                                                                      frames, e->K, X, W);
    if (e->ps.kind == LDPC_PARITY_STAIRCASE) {
        enc_rows_kernel<<<dim3(blocks(e->M), wt), kEncBlock, 0, s>>>(X, e->ptr.p, e->col.p, 0, e->M, P, W);
        enc_stair_local_kernel<<<dim3(blocks(e->chunks), wt), kEncBlock, 0, s>>>(e->M, P, e->aux.p, W);
        if (e->chunks > 1) {
            enc_stair_scan_kernel<<<wt, 64 * kEncScanWaves, 0, s>>>(e->aux.p, e->chunks, W);
            enc_stair_apply_kernel<<<dim3(blocks(e->M - kEncChunk), wt), kEncBlock, 0, s>>>(P, e->aux.p, e->M, W);
        }
    } else if (e->ps.kind == LDPC_PARITY_DENSE) {
        const int32_t rho = e->N - e->K;
        enc_rows_kernel<<<dim3(blocks(e->M), wt), kEncBlock, 0, s>>>(X, e->ptr.p, e->col.p, 0, e->M, e->aux.p, W);
        int32_t slices = 1;
        const int32_t slice_cols = enc_dense_slices(e->M, rho, W, &slices);
        if (slices > 1) LDPC_HIP_TRY(hipMemsetAsync(P, 0, (size_t)rho * W * sizeof(uint64_t), s));
        enc_dense_kernel<<<dim3((unsigned)((rho + kDenseRows - 1) / kDenseRows), wt, (unsigned)slices), kEncBlock, kDenseLds, s>>>(
            e->T.p, e->tw, e->aux.p, e->M, rho, P, W, slice_cols);
    } else {
        const int32_t core = e->ps.c * e->ps.z;
        enc_rows_kernel<<<dim3(blocks(core), wt), kEncBlock, 0, s>>>(X, e->ptr.p, e->col.p, 0, core, e->aux.p, W);
        enc_dd_core_kernel<<<dim3(blocks(e->ps.z), wt), kEncBlock, 0, s>>>(e->aux.p, P, e->ps.z, e->ps.c, e->ps.x, e->ps.a, e->ps.b, W);
        if (core < e->M)
            enc_rows_kernel<<<dim3(blocks(e->M - core), wt), kEncBlock, 0, s>>>(X, e->ptr.p, e->col.p, core, e->M, P, W);
    }
    const uintptr_t at = (uintptr_t)code_dev;
    const dim3 grid(blocks((e->N + 63) / 64), (unsigned)W);
    if (format == LDPC_CODE_BITS) {
        const int32_t align = (e->N % 16 == 0 && at % 16 == 0) ? 16 : (e->N % 4 == 0 && at % 4 == 0) ? 4 : 1;
        enc_store_kernel<1><<<grid, kEncBlock, 0, s>>>(X, e->N, W, frames, code_dev, align);
    } else {
        const int32_t align = ((e->N / 8) % 4 == 0 && at % 4 == 0) ? 4 : 1;
        enc_store_kernel<0><<<grid, kEncBlock, 0, s>>>(X, e->N, W, frames, code_dev, align);
    }
    LDPC_HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace

extern "C" {

int64_t ldpc_code_bytes(int32_t N, int64_t frames, int32_t format)
{
    if (N <= 0 || frames <= 0) return 0;
    if (format == LDPC_CODE_BITS) return frames * (int64_t)N;
    if (format == LDPC_CODE_PACKED && N % 8 == 0) return frames * (int64_t)(N / 8);
    return 0;
}

int ldpc_parity_structure(const ldpc_graph *g, int32_t K, int32_t block_rows, int32_t out[8])
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    ParityStructure ps;
    const int rc = analyse(g, K, block_rows, &ps);
    if (rc) return rc;
    out[0] = ps.kind; out[1] = ps.c; out[2] = ps.x; out[3] = ps.a; out[4] = ps.b; out[5] = ps.ext; out[6] = ps.z;
    return LDPC_OK;
}

int ldpc_encoder_create(const ldpc_graph *g, int32_t K, int32_t block_rows, int32_t max_frames, int32_t device,
                        ldpc_encoder **out)
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (max_frames <= 0) return set_error(LDPC_ERR_ARG, "max_frames = %d must be positive", max_frames);
    ParityStructure ps;
    int rc = analyse(g, K, block_rows, &ps);
    if (rc) return rc;
    if ((rc = ldpc::use_device(device, "the encoder"))) return rc;
    ldpc_encoder *e = new (std::nothrow) ldpc_encoder;
    if (!e) return set_error(LDPC_ERR_NOMEM, "out of memory");
    e->device = device; e->N = g->N; e->K = K; e->M = g->M; e->max_frames = max_frames; e->ps = ps;
    e->Wmax = (max_frames + 63) / 64;
    e->chunks = (g->M + ldpc::kEncChunk - 1) / ldpc::kEncChunk;
    /* rows of the core (and of a staircase) sum their information columns; an extension row sums everything but
     * its own parity column K + m */
    const int32_t core = ps.kind == LDPC_PARITY_STAIRCASE ? g->M : ps.c * ps.z;
    std::vector<int32_t> ptr((size_t)g->M + 1, 0), col;
    col.reserve((size_t)g->E);
    for (int32_t m = 0; m < g->M; ++m) {
        for (int32_t k = g->row_ptr[m]; k < g->row_ptr[m + 1]; ++k) {
            const int32_t n = g->cols[k];
            if (m < core ? n < K : n != K + m) col.push_back(n);
        }
        ptr[(size_t)m + 1] = (int32_t)col.size();
    }
    const size_t aux = (ps.kind == LDPC_PARITY_STAIRCASE ? (size_t)e->chunks : (size_t)core) * e->Wmax;
    hipError_t err = e->X.alloc((size_t)g->N * e->Wmax);
    if (err == hipSuccess) err = e->aux.alloc(aux);
    if (err == hipSuccess) err = e->ptr.upload(ptr);
    if (err == hipSuccess) err = e->col.upload(col);
    if (err != hipSuccess) {
        delete e;
        return set_error(err == hipErrorOutOfMemory ? LDPC_ERR_NOMEM : LDPC_ERR_HIP, "encoder buffers: %s", hipGetErrorString(err));
    }
    *out = e;
    return LDPC_OK;
}

int ldpc_graph_systematic_order(const ldpc_graph *g, int32_t *perm, int32_t *rank) { return ldpc::systematic_order(g, perm, rank); }

int ldpc_parity_dense(const ldpc_graph *g, int32_t K, int64_t out[4])
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    ldpc::DenseSolve ds;
    const int rc = ldpc::dense_analyse(g, K, false, &ds);
    out[0] = ds.rho; out[1] = ds.rank_hp; out[2] = ds.M; out[3] = ds.tw;
    return rc;
}

int ldpc_parity_dense_rows(const ldpc_graph *g, int32_t K, int32_t first, int32_t rows, uint64_t *t_out, int64_t words)
{
    if (!t_out) return set_error(LDPC_ERR_ARG, "t_out is NULL");
    ldpc::DenseSolve ds;
    const int rc = ldpc::dense_analyse(g, K, true, &ds);
    if (rc) return rc;
    if (first < 0 || rows < 0 || (int64_t)first + rows > ds.rho)
        return set_error(LDPC_ERR_ARG, "rows [%d, %d + %d) outside [0, rho = %d)", first, first, rows, ds.rho);
    if (words < (int64_t)rows * ds.tw)
        return set_error(LDPC_ERR_ARG, "words = %lld, %d rows of %d words need %lld", (long long)words, rows, ds.tw, (long long)((int64_t)rows * ds.tw));
    std::copy_n(ds.T.begin() + (size_t)first * ds.tw, (size_t)rows * ds.tw, t_out);
    return LDPC_OK;
}

int ldpc_encoder_create_dense(const ldpc_graph *g, int32_t K, int32_t max_frames, int32_t device, ldpc_encoder **out)
{
    if (!out) return set_error(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (max_frames <= 0) return set_error(LDPC_ERR_ARG, "max_frames = %d must be positive", max_frames);
    ldpc::DenseSolve ds;
    int rc = ldpc::dense_analyse(g, K, true, &ds);      /* arguments, the M cap, then the elimination */
    if (rc) return rc;
    if ((rc = ldpc::use_device(device, "the encoder"))) return rc;
    ldpc_encoder *e = new (std::nothrow) ldpc_encoder;
    if (!e) return set_error(LDPC_ERR_NOMEM, "out of memory");
    e->device = device; e->N = g->N; e->K = K; e->M = g->M; e->max_frames = max_frames; e->tw = ds.tw;
    e->ps.kind = LDPC_PARITY_DENSE;
    e->Wmax = (max_frames + 63) / 64;
    /* lambda = H_s u: every row sums its information columns */
    std::vector<int32_t> ptr((size_t)g->M + 1, 0), col;
    col.reserve((size_t)g->E);
    for (int32_t m = 0; m < g->M; ++m) {
        for (int32_t k = g->row_ptr[m]; k < g->row_ptr[m + 1]; ++k)
            if (g->cols[k] < K) col.push_back(g->cols[k]);
        ptr[(size_t)m + 1] = (int32_t)col.size();
    }
    hipError_t err = e->X.alloc((size_t)g->N * e->Wmax);
    if (err == hipSuccess) err = e->aux.alloc((size_t)g->M * e->Wmax);
    if (err == hipSuccess) err = e->T.upload(ds.T);
    if (err == hipSuccess) err = e->ptr.upload(ptr);
    if (err == hipSuccess) err = e->col.upload(col);
    if (err == hipSuccess)      /* up to 128 KiB of tables: above 64 KiB a launch must have opted in */
        err = hipFuncSetAttribute((const void *)ldpc::enc_dense_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldpc::kDenseLds);
    if (err != hipSuccess) {
        delete e;
        return set_error(err == hipErrorOutOfMemory ? LDPC_ERR_NOMEM : LDPC_ERR_HIP, "encoder buffers: %s", hipGetErrorString(err));
    }
    *out = e;
    return LDPC_OK;
}

int ldpc_encoder_destroy(ldpc_encoder *e)
{
    if (!e) return LDPC_OK;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    delete e;
    return LDPC_OK;
}

int ldpc_encode_device(ldpc_encoder *e, const uint8_t *src_dev, int64_t src_bytes, int64_t frames, uint8_t *code_dev,
                       int64_t code_bytes, int32_t format, void *stream)
{
    if (int rc = ldpc::known_code_format(format, "code format")) return rc;
    if (!e) return set_error(LDPC_ERR_ARG, "encoder is NULL");
    if (!src_dev || !code_dev) return set_error(LDPC_ERR_ARG, "src_dev/code_dev is NULL");
    if (format == LDPC_CODE_PACKED && e->N % 8) return set_error(LDPC_ERR_ARG, "LDPC_CODE_PACKED needs N %% 8 == 0 (N = %d)", e->N);
    if (frames < 0 || frames > e->max_frames) return set_error(LDPC_ERR_ARG, "frames = %lld outside [0, max_frames = %d]", (long long)frames, e->max_frames);
    if (frames == 0) return LDPC_OK;
    if (src_bytes <= 0 || (frames - 1) * (int64_t)e->K / 8 >= src_bytes)
        return set_error(LDPC_ERR_ARG, "frame %lld starts at byte %lld, beyond src_bytes = %lld", (long long)(frames - 1),
                         (long long)((frames - 1) * (int64_t)e->K / 8), (long long)src_bytes);
    if (code_bytes < ldpc_code_bytes(e->N, frames, format))
        return set_error(LDPC_ERR_ARG, "code_bytes = %lld, %lld frames need %lld", (long long)code_bytes, (long long)frames,
                         (long long)ldpc_code_bytes(e->N, frames, format));
    LDPC_HIP_TRY(hipSetDevice(e->device));
    return enqueue(e, src_dev, src_bytes, 0, frames, code_dev, format, (hipStream_t)stream);
}

int ldpc_encode(ldpc_encoder *e, const uint8_t *src_host, int64_t src_bytes, uint8_t *code_host, int64_t code_bytes)
{
    if (!e) return set_error(LDPC_ERR_ARG, "encoder is NULL");
    if (!src_host || !code_host || src_bytes <= 0) return set_error(LDPC_ERR_ARG, "src_host/code_host is NULL or src_bytes <= 0");
    if (e->N % 8) return set_error(LDPC_ERR_ARG, "ldpc_encode writes LDPC_CODE_PACKED: needs N %% 8 == 0 (N = %d)", e->N);
    if (e->K < 8) return set_error(LDPC_ERR_ARG, "K = %d: a frame reads no whole source byte", e->K);
    const int64_t K = e->K, nb = e->N / 8;
    /* the last frame is the first one with (f + 1) K / 8 >= src_bytes (Coder::encode) */
    int64_t last = (src_bytes * 8) / K;
    while (last > 0 && last * K / 8 >= src_bytes) --last;
    while ((last + 1) * K / 8 < src_bytes) ++last;
    const int64_t frames = last + 1;
    if (code_bytes < frames * nb)
        return set_error(LDPC_ERR_ARG, "code_bytes = %lld, %lld frames need %lld", (long long)code_bytes, (long long)frames, (long long)(frames * nb));
    LDPC_HIP_TRY(hipSetDevice(e->device));
    if (!e->src_stage.p) LDPC_HIP_TRY(e->src_stage.alloc((size_t)((int64_t)e->max_frames * K / 8 + K / 8 + 1)));
    if (!e->code_stage.p) LDPC_HIP_TRY(e->code_stage.alloc((size_t)(e->max_frames * nb)));
    for (int64_t f0 = 0; f0 < frames; f0 += e->max_frames) {
        const int64_t n = std::min<int64_t>(e->max_frames, frames - f0);
        const int64_t base = f0 * K / 8;
        const int64_t bytes = std::min<int64_t>(src_bytes, (f0 + n - 1) * K / 8 + K / 8) - base;
        LDPC_HIP_TRY(hipMemcpy(e->src_stage.p, src_host + base, (size_t)bytes, hipMemcpyHostToDevice));
        const int rc = enqueue(e, e->src_stage.p, bytes, f0, n, e->code_stage.p, LDPC_CODE_PACKED, nullptr);
        if (rc) return rc;
        LDPC_HIP_TRY(hipMemcpy(code_host + f0 * nb, e->code_stage.p, (size_t)(n * nb), hipMemcpyDeviceToHost));
    }
    return LDPC_OK;
}

}  // extern "C"

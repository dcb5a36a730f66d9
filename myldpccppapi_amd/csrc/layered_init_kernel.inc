/* layered_init_kernel.inc -- kernel body included by layered_kernels.hpp into layered_init_kernel and
 * layered_init_scaled_kernel, so that both are compiled from one text and the first exactly as before.  IN: element type
 * of the caller's buffer; a narrow one goes through llr_patch_fill (llr_input.hpp), float through the loop below. */
    constexpr int F = 64 * V;
    constexpr int LD = F + 1;
    __shared__ float patch[kInitCols * LD];
    const int tile = blockIdx.y;
    const int n0 = blockIdx.x * kInitCols;
    const IN *__restrict__ llr = static_cast<const IN *>(a.llr);
    if constexpr (!std::is_same<IN, float>::value) {
        llr_patch_fill<IN, F, LD, kInitCols, kBlock, SCALED>(patch, llr, a.llr_unit, a.frames, a.N, tile, n0, scale);
    } else {
        const int c = threadIdx.x & (kInitCols - 1);
        const int n = n0 + c;
        for (int f = threadIdx.x / kInitCols; f < F; f += kBlock / kInitCols) {
            const int64_t frame = (int64_t)tile * F + f;
            float y = 1.0f;
            if (frame < a.frames && n < a.N) y = llr[(size_t)frame * a.N + n];
            if (SCALED) y = scale * y;
            patch[c * LD + f] = y;
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int c = threadIdx.x >> 6; c < kInitCols; c += kWavesPerBlock) {
        const int n = n0 + c;
        if (n >= a.N) break;
        float y[V];
#pragma unroll
        for (int v = 0; v < V; ++v) y[v] = patch[c * LD + lane * V + v];
        vstore<V>(a.P + ((size_t)tile * a.N + n) * F + (size_t)lane * V, y);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const uint64_t w = __ballot(y[v] < 0.0f);
            if (lane == 0) a.hard[((size_t)tile * a.N + n) * V + v] = a.zero_bits ? 0ull : w;
        }
    }

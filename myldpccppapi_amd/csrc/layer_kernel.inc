/* layer_kernel.inc -- kernel body included by layered_kernels.hpp into layer_kernel and layer_corr_kernel,
 * so that both are compiled from one text and layer_kernel exactly as before. */
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.y;
    if (tile_finished<V>(a.done, tile)) return;
    const int wave = (int)blockIdx.x * kWavesPerBlock + wave_id_in_block();
    const int r_begin = wave * a.rows_per_wave;
    const int r_end = min(r_begin + a.rows_per_wave, a.n_rows);
    float *Pt = a.P + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
    float *Rt = a.R + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    uint64_t *hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
    uint64_t frozen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];

    for (int r = r_begin; r < r_end; ++r) {
        const int e0 = a.cls_e0[r];
        int col[D];
#pragma unroll
        for (int k = 0; k < D; ++k) col[k] = a.edge_col[e0 + k];
        float p[D][V], m[D][V];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            vload<V>(m[k], Rt + (size_t)(e0 + k) * F);
            vload<V>(p[k], Pt + (size_t)col[k] * F);
        }
        if (HOST) {
#pragma unroll
            for (int k = 0; k < D; ++k)
#pragma unroll
                for (int v = 0; v < V; ++v) p[k][v] = p[k][v] - m[k][v];      /* refreshQTDMP */
            check_ms<D, V>(p, m);                                                 /* refreshRTDMP */
#pragma unroll
            for (int k = 0; k < D; ++k) {
#pragma unroll
                for (int v = 0; v < V; ++v) p[k][v] = p[k][v] + m[k][v];      /* refreshPostPTDMP */
                vstore<V>(Rt + (size_t)(e0 + k) * F, m[k]);
                vstore<V>(Pt + (size_t)col[k] * F, p[k]);
            }
            continue;
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float prod = 1.0f, b = 1000.0f, c = 1001.0f;   /* decodeCL.c:346-348 */
            int bind = -1;
            float sg[D];
#pragma unroll
            for (int k = 0; k < D; ++k) {                  /* :350-367 */
                const float q = p[k][v] - m[k][v];
                sg[k] = cl_sign(q);
                prod *= q;
                p[k][v] = q;
                const float mag = __builtin_fabsf(q);
                if (mag <= b) { c = b; b = mag; bind = k; }
                else if (mag > b && mag <= c) { c = mag; }
            }
            if (CORR) { b = ms_corr<float>(b, corr); c = ms_corr<float>(c, corr); }   /* once per row */
            const float sa = cl_sign(prod);                /* :369 */
            const float ab = sa * b, ac = sa * c;
#pragma unroll
            for (int k = 0; k < D; ++k) {                  /* :371-383 */
                const float rn = sg[k] * ((k == bind) ? ac : ab);
                m[k][v] = rn;
                p[k][v] = p[k][v] + rn;
            }
        }
#pragma unroll
        for (int k = 0; k < D; ++k) {
            vstore<V>(Rt + (size_t)(e0 + k) * F, m[k]);
            vstore<V>(Pt + (size_t)col[k] * F, p[k]);
#pragma unroll
            for (int v = 0; v < V; ++v) {                  /* :388-389, kept current per write */
                const uint64_t w = __ballot(p[k][v] < 0.0f);
                if (lane == 0) {
                    const uint64_t old = hard_t[(size_t)col[k] * V + v];
                    hard_t[(size_t)col[k] * V + v] = (old & frozen[v]) | (w & ~frozen[v]);
                }
            }
        }
    }

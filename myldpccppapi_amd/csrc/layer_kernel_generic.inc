/* layer_kernel_generic.inc -- kernel body included by layered_kernels.hpp into layer_kernel_generic and
 * layer_corr_kernel_generic, so that both are compiled from one text and the first exactly as before. */
    constexpr size_t F = 64 * V;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.y;
    if (tile_finished<V>(a.done, tile)) return;
    const int wave = (int)blockIdx.x * kWavesPerBlock + wave_id_in_block();
    const int r_begin = wave * a.rows_per_wave;
    const int r_end = min(r_begin + a.rows_per_wave, a.n_rows);
    const int D = a.degree;
    float *Pt = a.P + (size_t)tile * (size_t)a.N * F + (size_t)lane * V;
    float *Rt = a.R + (size_t)tile * (size_t)a.E * F + (size_t)lane * V;
    uint64_t *hard_t = a.hard + (size_t)tile * (size_t)a.N * V;
    uint64_t frozen[V];
#pragma unroll
    for (int v = 0; v < V; ++v) frozen[v] = a.done[(size_t)tile * V + v];

    for (int r = r_begin; r < r_end; ++r) {
        const int e0 = a.cls_e0[r];
        float prod[V], b[V], c[V], sa[V];
        int bind[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { prod[v] = 1.0f; b[v] = 1000.0f; c[v] = 1001.0f; bind[v] = -1; }
        for (int k = 0; k < D; ++k) {
            const int col = a.edge_col[e0 + k];
            float m[V], p[V];
            vload<V>(m, Rt + (size_t)(e0 + k) * F);
            vload<V>(p, Pt + (size_t)col * F);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float q = p[v] - m[v];
                prod[v] *= q;
                p[v] = q;
                const float mag = __builtin_fabsf(q);
                if (mag <= b[v]) { c[v] = b[v]; b[v] = mag; bind[v] = k; }
                else if (mag > b[v] && mag <= c[v]) { c[v] = mag; }
            }
            vstore<V>(Pt + (size_t)col * F, p);        /* q parked in P, as decodeCL.c:357 */
        }
        if (CORR) {
#pragma unroll
            for (int v = 0; v < V; ++v) { b[v] = ms_corr<float>(b[v], corr); c[v] = ms_corr<float>(c[v], corr); }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) sa[v] = cl_sign(prod[v]);
        for (int k = 0; k < D; ++k) {
            const int col = a.edge_col[e0 + k];
            float q[V], rn[V];
            vload<V>(q, Pt + (size_t)col * F);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                rn[v] = cl_sign(q[v]) * ((k == bind[v]) ? sa[v] * c[v] : sa[v] * b[v]);
                q[v] = q[v] + rn[v];
            }
            vstore<V>(Rt + (size_t)(e0 + k) * F, rn);
            vstore<V>(Pt + (size_t)col * F, q);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const uint64_t w = __ballot(q[v] < 0.0f);
                if (lane == 0) {
                    const uint64_t old = hard_t[(size_t)col * V + v];
                    hard_t[(size_t)col * V + v] = (old & frozen[v]) | (w & ~frozen[v]);
                }
            }
        }
    }

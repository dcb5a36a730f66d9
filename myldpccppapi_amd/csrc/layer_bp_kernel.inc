/* layer_bp_kernel.inc -- body of layer_bp_kernel<D, V> (layered_kernels.hpp): layer_kernel.inc's frame with check_bp
 * as the row.  One load and one store of R and of P per edge; p holds q, m holds the row's output. */
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
#pragma unroll
        for (int k = 0; k < D; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) p[k][v] = p[k][v] - m[k][v];          /* q_k */
        check_bp<D, V, float>(p, m);                                              /* R_k = out_k */
#pragma unroll
        for (int k = 0; k < D; ++k) {
#pragma unroll
            for (int v = 0; v < V; ++v) p[k][v] = p[k][v] + m[k][v];          /* P = q_k + R_k */
            vstore<V>(Rt + (size_t)(e0 + k) * F, m[k]);
            vstore<V>(Pt + (size_t)col[k] * F, p[k]);
#pragma unroll
            for (int v = 0; v < V; ++v) {                  /* bits kept current per write, as layer_kernel does */
                const uint64_t w = __ballot(p[k][v] < 0.0f);
                if (lane == 0) {
                    const uint64_t old = hard_t[(size_t)col[k] * V + v];
                    hard_t[(size_t)col[k] * V + v] = (old & frozen[v]) | (w & ~frozen[v]);
                }
            }
        }
    }

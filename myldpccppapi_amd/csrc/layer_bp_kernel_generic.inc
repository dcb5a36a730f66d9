/* layer_bp_kernel_generic.inc -- body of layer_bp_kernel_generic<V> (layered_kernels.hpp): check_bp's association with
 * run-time loops over a row that is updated in place.
 *
 * Invariant: when step k begins, edges 0 .. k-1 of the row hold their new R and P, edges k .. D-1 their old ones.  Step k
 * reads q_j = P[col_j] - R_j only for j >= k -- q_k itself and, for b_{k+1}, the j > k -- and takes everything it needs
 * of the j < k from f = f_{k-1}, carried in registers and formed from q_{k-1} BEFORE step k-1 stored.  A row's columns
 * are distinct (edges ascend strictly within a row) and rows of a layer share no column (layered_plan_create), so what
 * step k stores at R_k and P[col_k] is read by no other edge of this row and by no other row of this launch. */
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
        /* t_j = bp_clamp(q_j) of an edge that still holds its old values */
        auto load_t = [&](int j, float (&t)[V]) {
            float pj[V], mj[V];
            vload<V>(mj, Rt + (size_t)(e0 + j) * F);
            vload<V>(pj, Pt + (size_t)a.edge_col[e0 + j] * F);
#pragma unroll
            for (int v = 0; v < V; ++v) t[v] = bp_clamp(pj[v] - mj[v]);
        };
        float f[V];
#pragma unroll
        for (int v = 0; v < V; ++v) f[v] = 0.0f;
        for (int k = 0; k < D; ++k) {
            const int col = a.edge_col[e0 + k];
            float q[V], o[V];
            {
                float mk[V];
                vload<V>(mk, Rt + (size_t)(e0 + k) * F);
                vload<V>(q, Pt + (size_t)col * F);
#pragma unroll
                for (int v = 0; v < V; ++v) q[v] = q[v] - mk[v];
            }
            if (D == 1) {
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = 1000.0f;
            } else if (k == D - 1) {
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = f[v];                       /* f_{D-2} */
            } else {
                float b[V], t[V];
                load_t(D - 1, b);
                for (int j = D - 2; j > k; --j) {
                    load_t(j, t);
#pragma unroll
                    for (int v = 0; v < V; ++v) b[v] = bp_boxplus(t[v], b[v]);   /* b_j = t_j [+] b_{j+1} */
                }
#pragma unroll
                for (int v = 0; v < V; ++v) o[v] = (k == 0) ? b[v] : bp_boxplus(f[v], b[v]);
            }
#pragma unroll
            for (int v = 0; v < V; ++v) {                   /* f_k from q_k, before edge k is stored */
                const float tk = bp_clamp(q[v]);
                f[v] = (k == 0) ? tk : bp_boxplus(f[v], tk);
                q[v] = q[v] + o[v];
            }
            vstore<V>(Rt + (size_t)(e0 + k) * F, o);
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

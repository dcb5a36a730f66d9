/* ldsp_layered_kernel.inc -- kernel body included by ldsp_kernels.hpp into the plain and the corrected (CORR) kernel,
 * so that both are compiled from one text and the plain kernel exactly as before. */
    extern __shared__ float lds[];
    float *P = lds;                                                             /* [lds_cols][z] */
    const int r = (int)threadIdx.x, LANES = (int)blockDim.x;
    const int z = a.z;
    uint32_t *wg_flag = reinterpret_cast<uint32_t *>(lds + (((size_t)a.lds_cols * z + 1) & ~(size_t)1));
    const bool row = r < z;
    const size_t ring = (size_t)blockIdx.x * ((size_t)a.layers * z) + r;        /* [layer][z], mine: + r */
    uint4 *recs = a.recs + ring;
    uint32_t *zfs = a.zf + ring;
    const ldpc_const_i32 hdr = as_constant(a.hdr), pack = as_constant(a.pack), cslot = as_constant(a.col_slot);
    /* OR over the workgroup through one LDS word (no static LDS: P sits at LDS address 0 and the
     * table's byte offsets are final addresses) */
    auto wg_any = [&](bool pred) {
        if (r == 0) *wg_flag = 0u;
        lds_barrier();
        if (__ballot(pred) != 0ull && (r & 63) == 0) *wg_flag = 1u;
        lds_barrier();
        const uint32_t f = *wg_flag;
        lds_barrier();                                             /* before the word is cleared again */
        return f != 0u;
    };
    for (int64_t frame = blockIdx.x; frame < a.frames; frame += gridDim.x) {
        const float *y = a.llr + (size_t)frame * a.N;
        if (row) {
            for (int bc = 0; bc < a.nb; ++bc) {
                const int slot = cslot[bc];
                if (slot >= 0) P[slot * z + r] = y[bc * z + r];
            }
            /* iteration 0: R = 0 (|ab| = |ac| = 0, signs +); an external column starts from its
             * channel value.  Written to the ring so that every layer step finds its record there. */
            for (int l = 0; l < a.layers; ++l) {
                uint4 rec = uint4{0u, 0u, 0u, 0u};
                if (hdr[l * 4 + 1]) rec.w = __float_as_uint(y[hdr[l * 4 + 2] + ldsp_wrap(r, hdr[l * 4 + 3], z)]);
                recs[(size_t)l * z] = rec;
            }
        }
        uint4 cur = uint4{0u, 0u, 0u, 0u};
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
#define LDPC_LDSP_CASE(D) case D + 1: par = ldsp_row_parity<D + 1>(P, pk, z, r); break;
                LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
            default: break;
            }
            /* hard decision of the layer's external column: its posterior is in my record */
            if (ext) par ^= __ballot(__uint_as_float(recs[(size_t)l * z].w) < 0.0f);
            return par;
        };
        while (true) {
            for (int l = 0; l < a.layers; ++l) {
                /* the next layer step's record (wrapping into the next iteration), requested before
                 * this step's work; with a single layer it is this step's own output */
                const int ln = l + 1 < a.layers ? l + 1 : 0;
                /* by every lane, outside any branch: a conditional request makes the compiler copy the
                 * registers, and wait for them, where the branch ends -- at once.  Lanes beyond the last row
                 * read their neighbours' records (the rings end with spare ones). */
                uint4 nxt = recs[(size_t)ln * z];
                const int dl = hdr[l * 4], ext = hdr[l * 4 + 1];
                const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                uint4 rec = uint4{0u, 0u, 0u, 0u};
                if (row) {
                    uint32_t par = 0;                               /* (ldsp_row_any's; not used here) */
                    bool done = false;
                    if (ext) {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D: done = ldsp_row<D, 1, true, false, CORR>(P, pk, z, r, cur, &rec, &par, corr); break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    } else {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D + 1: done = ldsp_row<D + 1, 0, true, false, CORR>(P, pk, z, r, cur, &rec, &par, corr); break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    }
                    if (!done) rec = ldsp_row_any<CORR>(P, pk, dl, ext, z, r, cur, zfs + (size_t)l * z, &par, corr);
                }
                /* the requested record has had this step's work to arrive: take it -- on every path, not
                 * inside the branch above -- BEFORE the store below is issued, or the wait for it would
                 * cover the store as well and put a full memory round trip into every layer step */
                asm volatile("" : "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w) : : "memory");
                if (row) recs[(size_t)l * z] = rec;
                if (a.layers == 1) nxt = rec;
                lds_barrier();
                cur = nxt;
            }
            /* syndrome of the hard decisions: every round when a clean frame stops early, else only
             * after the last one (its only use then is the frame's converged flag) */
            ++time;
            int any_bad = 1;
            if (a.early_term || time == a.rounds) {
                /* the rows of the last layer first (their columns are in the iteration's final state like all
                 * others, but a frame that has not converged nearly always shows it there already): only
                 * when all of them are even the other layers are looked at.  The row code does not
                 * keep parities: one layer's worth of reads here is cheaper than an instruction per edge. */
                uint64_t bad = row ? layer_odd(a.layers - 1) : 0ull;
                if (!wg_any(bad != 0ull)) {
                    if (row)
                        for (int l = 0; l + 1 < a.layers; ++l) bad |= layer_odd(l);
                    any_bad = wg_any(bad != 0ull) ? 1 : 0;
                }
            }
            clean = !any_bad;
            if ((clean && a.early_term) || time == a.rounds) break;
        }
        /* toChar (decodeCL.c:414-423): the information columns sit in LDS at slot = block column */
        const int64_t base = frame * (int64_t)a.K / 8;
        for (int j = r; j < a.K / 8; j += LANES) {
            unsigned byte = 0;
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) byte |= (P[j * 8 + bit] < 0.0f ? 1u : 0u) << bit;
            if (base + j < a.out_bytes) a.out[base + j] = (uint8_t)byte;
        }
        if (a.dump_p && row) {
            for (int bc = 0; bc < a.nb; ++bc) {
                const int slot = cslot[bc];
                if (slot >= 0) a.dump_p[(size_t)frame * a.N + bc * z + r] = P[slot * z + r];
            }
            for (int l = 0; l < a.layers; ++l)
                if (hdr[l * 4 + 1])
                    a.dump_p[(size_t)frame * a.N + hdr[l * 4 + 2] + ldsp_wrap(r, hdr[l * 4 + 3], z)] =
                        __uint_as_float(recs[(size_t)l * z].w);
        }
        if (a.dump_r && row) {
            for (int l = 0; l < a.layers; ++l) {
                const int d = hdr[l * 4] + hdr[l * 4 + 1], e0 = a.layer_e0[l];
                const uint4 rec = recs[(size_t)l * z];
                const uint32_t zf = (rec.z & kLdspIrregular) ? zfs[(size_t)l * z] : 0u;
                for (int k = 0; k < d; ++k)
                    a.dump_r[(size_t)frame * a.E + e0 + r * d + k] = __uint_as_float(ldsp_old_message(rec, zf, k, d));
            }
        }
        if (r == 0) {
            const int it = clean ? time : a.max_iter;
            if (a.iters) a.iters[frame] = it;
            atomicMax(&a.summary[0], it);
            if (clean) atomicAdd(&a.summary[1], 1);
        }
        __syncthreads();                                           /* P is refilled for the next frame */
    }

/* ldsp_flood_kernel.inc -- kernel body included by ldsp_kernels.hpp into the plain and the corrected (CORR) kernel,
 * so that both are compiled from one text and the plain kernel exactly as before. */
    extern __shared__ float lds[];
    const int r = (int)threadIdx.x, LANES = (int)blockDim.x, MW = LANES >> 6, wave = r >> 6;
    const int z = a.z;
    const size_t image = ((size_t)a.lds_cols * z + 1) & ~(size_t)1;
    float *Pa = lds, *Pb = lds + image;                             /* old / new posteriors, [lds_cols][z] each */
    uint64_t *extneg = reinterpret_cast<uint64_t *>(lds + 2 * image);   /* [layers][MW] */
    uint32_t *wg_flag = reinterpret_cast<uint32_t *>(extneg + (size_t)a.layers * MW);
    const bool row = r < z;
    uint4 *recs = a.recs + (size_t)blockIdx.x * ((size_t)a.layers * z) + r;
    uint32_t *zfs = a.zf + (size_t)blockIdx.x * ((size_t)a.layers * z) + r;
    const ldpc_const_i32 hdr = as_constant(a.hdr), pack = as_constant(a.pack), cslot = as_constant(a.col_slot);
    auto wg_any = [&](bool pred) {
        if (r == 0) *wg_flag = 0u;
        lds_barrier();
        if (__ballot(pred) != 0ull && (r & 63) == 0) *wg_flag = 1u;
        lds_barrier();
        const uint32_t f = *wg_flag;
        lds_barrier();
        return f != 0u;
    };
    auto fill = [&](float *P, const float *y) {                    /* the LDS-resident columns' channel values */
        if (row)
            for (int bc = 0; bc < a.nb; ++bc) {
                const int slot = cslot[bc];
                if (slot >= 0) P[slot * z + r] = y[bc * z + r];
            }
    };
    for (int64_t frame = blockIdx.x; frame < a.frames; frame += gridDim.x) {
        const float *y = a.llr + (size_t)frame * a.N;
        fill(Pa, y);                                               /* Q_0 = y: P_0 = y, R_0 = 0 */
        int time = 0;
        bool clean = false;
        uint4 cur = uint4{0u, 0u, 0u, 0u};
        while (true) {
            fill(Pb, y);                                           /* refreshPostPMS starts from the channel value */
            __syncthreads();
            uint64_t last_bad = 0;
            for (int l = 0; l < a.layers; ++l) {
                const int ln = l + 1 < a.layers ? l + 1 : 0;
                uint4 nxt = uint4{0u, 0u, 0u, 0u};
                if (row && a.layers > 1 && (time > 0 || ln == 0)) nxt = recs[(size_t)ln * z];
                const int dl = hdr[l * 4], ext = hdr[l * 4 + 1];
                const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                if (row) {
                    float yext = 0.0f;
                    if (ext) yext = y[hdr[l * 4 + 2] + ldsp_wrap(r, hdr[l * 4 + 3], z)];
                    const float pext_old = time == 0 ? yext : __uint_as_float(cur.w);
                    uint4 rec = cur;
                    uint64_t pm = 0, em = 0;
                    bool done = CHAIN;                             /* the chain arithmetic has no slow path */
                    if (ext) {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D:                                                                                  \
                            if (CHAIN) ldsp_flood_row<D, 1, CORR>(Pa, Pb, pk, z, r, cur, pext_old, yext, &rec, &pm, &em, corr);        \
                            else done = ldsp_mscl_row<D, 1>(Pa, Pb, pk, z, r, cur, pext_old, yext, &rec, &pm, &em);         \
                            break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    } else {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D + 1:                                                                              \
                            if (CHAIN) ldsp_flood_row<D + 1, 0, CORR>(Pa, Pb, pk, z, r, cur, 0.0f, 0.0f, &rec, &pm, &em, corr);        \
                            else done = ldsp_mscl_row<D + 1, 0>(Pa, Pb, pk, z, r, cur, 0.0f, 0.0f, &rec, &pm, &em);         \
                            break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    }
                    if (!CHAIN && !done)
                        rec = ldsp_mscl_row_any(Pa, Pb, pk, dl, ext, z, r, cur, pext_old, yext, zfs + (size_t)l * z, &pm, &em);
                    if (ext && (r & 63) == 0) extneg[l * MW + wave] = em;
                    last_bad = pm;
                    asm volatile("" : "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w) : : "memory");
                    recs[(size_t)l * z] = rec;
                    if (a.layers == 1) nxt = rec;
                }
                lds_barrier();
                cur = nxt;
            }
            ++time;
            int any_bad = 1;
            /* the last layer's rows have just written the final posteriors of their columns */
            if ((a.early_term || time == a.rounds) && !wg_any(row && last_bad != 0ull)) {
                uint64_t bad = 0;
                if (row) {
                    for (int l = 0; l < a.layers; ++l) {
                        const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                        uint64_t par = 0;
                        switch (hdr[l * 4]) {
#define LDPC_LDSP_CASE(D) case D: par = ldsp_flood_parity<D, CHAIN>(Pb, pk, z, r); break;
                            LDPC_LDSP_WIDTHS1(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                        if (hdr[l * 4 + 1]) par ^= extneg[l * MW + wave];
                        bad |= par;
                    }
                }
                any_bad = wg_any(bad != 0ull) ? 1 : 0;
            }
            clean = !any_bad;
            float *t = Pa; Pa = Pb; Pb = t;                         /* the new posteriors are the next round's old ones */
            if ((clean && a.early_term) || time == a.rounds) break;
        }
        /* Pa holds the final posteriors; the information columns sit at slot = block column */
        const int64_t base = frame * (int64_t)a.K / 8;
        for (int j = r; j < a.K / 8; j += LANES) {
            unsigned byte = 0;
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) byte |= (ldsp_flood_bit<CHAIN>(Pa[j * 8 + bit]) ? 1u : 0u) << bit;
            if (base + j < a.out_bytes) a.out[base + j] = (uint8_t)byte;
        }
        if (a.dump_p && row) {
            for (int bc = 0; bc < a.nb; ++bc) {
                const int slot = cslot[bc];
                if (slot >= 0) a.dump_p[(size_t)frame * a.N + bc * z + r] = Pa[slot * z + r];
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
        __syncthreads();
    }

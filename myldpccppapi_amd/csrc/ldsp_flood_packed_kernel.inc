/* ldsp_flood_packed_kernel.inc -- kernel body included by ldsp_kernels.hpp into the plain and the corrected (CORR) kernel,
 * so that both are compiled from one text and the plain kernel exactly as before. */
    extern __shared__ float lds[];
    const int lane = (int)threadIdx.x;
    const int z = a.z;
    const int g = lane / z, r = lane - g * z;
    const bool member = g < G;
    const size_t image = ((size_t)a.N + 1) & ~(size_t)1;
    float *Pa = lds + (size_t)(member ? g : 0) * 2 * image, *Pb = Pa + image;
    uint4 *recs = a.recs + ((size_t)blockIdx.x * G + (member ? g : 0)) * ((size_t)a.layers * z) + r;
    uint32_t *zfs = a.zf + ((size_t)blockIdx.x * G + (member ? g : 0)) * ((size_t)a.layers * z) + r;
    const ldpc_const_i32 hdr = as_constant(a.hdr), pack = as_constant(a.pack);
    const uint64_t gmask = (z >= 64 ? ~0ull : ((1ull << z) - 1ull)) << (member ? g * z : 0);
    for (int64_t frame0 = (int64_t)blockIdx.x * G; frame0 < a.frames; frame0 += (int64_t)gridDim.x * G) {
        const int64_t frame = frame0 + g;
        const bool mine = member && frame < a.frames;
        const float *y = a.llr + (size_t)(mine ? frame : 0) * a.N;
        if (mine)
            for (int n = r; n < a.N; n += z) Pa[n] = y[n];
        int time = 0, my_iters = a.max_iter;
        bool active = mine, clean = false;
        uint4 cur = uint4{0u, 0u, 0u, 0u};
        while (__ballot(active) != 0ull) {
            if (active)
                for (int n = r; n < a.N; n += z) Pb[n] = y[n];
            lds_barrier();
            uint64_t last_bad = 0;
            for (int l = 0; l < a.layers; ++l) {
                const int ln = l + 1 < a.layers ? l + 1 : 0;
                uint4 nxt = uint4{0u, 0u, 0u, 0u};
                if (active && a.layers > 1 && (time > 0 || ln == 0)) nxt = recs[(size_t)ln * z];
                const int d = hdr[l * 4];
                const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                if (active) {
                    uint4 rec = cur;
                    uint64_t pm = 0, em = 0;
                    bool done = CHAIN;
                    switch (d) {
#define LDPC_LDSP_CASE(D) case D:                                                                                  \
                        if (CHAIN) ldsp_flood_row<D, 0, CORR>(Pa, Pb, pk, z, r, cur, 0.0f, 0.0f, &rec, &pm, &em, corr);                \
                        else done = ldsp_mscl_row<D, 0>(Pa, Pb, pk, z, r, cur, 0.0f, 0.0f, &rec, &pm, &em);                 \
                        break;
                        LDPC_LDSP_WIDTHS1(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                    default: break;
                    }
                    if (!CHAIN && !done)
                        rec = ldsp_mscl_row_any(Pa, Pb, pk, d, 0, z, r, cur, 0.0f, 0.0f, zfs + (size_t)l * z, &pm, &em);
                    last_bad = pm;
                    asm volatile("" : "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w) : : "memory");
                    recs[(size_t)l * z] = rec;
                    if (a.layers == 1) nxt = rec;
                }
                lds_barrier();
                cur = nxt;
            }
            ++time;
            const bool check = a.early_term || time == a.rounds;
            bool any_bad = true;
            const bool need = active && check && (last_bad & gmask) == 0ull;
            if (__ballot(need) != 0ull) {
                uint64_t bad = 0;
                if (need) {
                    for (int l = 0; l < a.layers; ++l) {
                        const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                        switch (hdr[l * 4]) {
#define LDPC_LDSP_CASE(D) case D: bad |= ldsp_flood_parity<D, CHAIN>(Pb, pk, z, r); break;
                            LDPC_LDSP_WIDTHS1(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    }
                    any_bad = (bad & gmask) != 0ull;
                }
            }
            if (active) {
                clean = check && !any_bad;
                float *t = Pa; Pa = Pb; Pb = t;
                if ((clean && a.early_term) || time == a.rounds) {
                    active = false;
                    my_iters = clean ? time : a.max_iter;
                }
            }
            lds_barrier();
        }
        if (mine) {
            const int64_t base = frame * (int64_t)a.K / 8;
            for (int j = r; j < a.K / 8; j += z) {
                unsigned byte = 0;
#pragma unroll
                for (int bit = 0; bit < 8; ++bit) byte |= (ldsp_flood_bit<CHAIN>(Pa[j * 8 + bit]) ? 1u : 0u) << bit;
                if (base + j < a.out_bytes) a.out[base + j] = (uint8_t)byte;
            }
            if (a.dump_p)
                for (int n = r; n < a.N; n += z) a.dump_p[(size_t)frame * a.N + n] = Pa[n];
            if (a.dump_r) {
                for (int l = 0; l < a.layers; ++l) {
                    const int d = hdr[l * 4], e0 = a.layer_e0[l];
                    const uint4 rec = recs[(size_t)l * z];
                    const uint32_t zf = (rec.z & kLdspIrregular) ? zfs[(size_t)l * z] : 0u;
                    for (int k = 0; k < d; ++k)
                        a.dump_r[(size_t)frame * a.E + e0 + r * d + k] = __uint_as_float(ldsp_old_message(rec, zf, k, d));
                }
            }
            if (r == 0) {
                if (a.iters) a.iters[frame] = my_iters;
                atomicMax(&a.summary[0], my_iters);
                if (clean) atomicAdd(&a.summary[1], 1);
            }
        }
        lds_barrier();
    }

/* ldsp_layered_packed_kernel.inc -- kernel body included by ldsp_kernels.hpp into the plain and the corrected (CORR) kernel,
 * so that both are compiled from one text and the plain kernel exactly as before. */
    extern __shared__ float lds[];
    const int lane = (int)threadIdx.x;
    const int z = a.z;
    const int g = lane / z, r = lane - g * z;
    const bool member = g < G;                                      /* lane belongs to a frame slot */
    const size_t frame_floats = ((size_t)a.lds_cols * z + 1) & ~(size_t)1;
    float *P = lds + (size_t)(member ? g : 0) * frame_floats;       /* [lds_cols][z] of my frame */
    uint64_t *extneg = reinterpret_cast<uint64_t *>(lds + (size_t)G * frame_floats);   /* [layers] lane masks */
    const size_t ring = ((size_t)blockIdx.x * G + (member ? g : 0)) * ((size_t)a.layers * z) + r;
    uint4 *recs = a.recs + ring;
    uint32_t *zfs = a.zf + ring;
    const ldpc_const_i32 hdr = as_constant(a.hdr), pack = as_constant(a.pack), cslot = as_constant(a.col_slot);
    const uint64_t gmask = (z >= 64 ? ~0ull : ((1ull << z) - 1ull)) << (member ? g * z : 0);
    for (int64_t frame0 = (int64_t)blockIdx.x * G; frame0 < a.frames; frame0 += (int64_t)gridDim.x * G) {
        const int64_t frame = frame0 + g;
        const bool mine = member && frame < a.frames;
        const float *y = a.llr + (size_t)(mine ? frame : 0) * a.N;
        if (mine) {
            for (int bc = 0; bc < a.nb; ++bc) {
                const int slot = cslot[bc];
                if (slot >= 0) P[slot * z + r] = y[bc * z + r];
            }
            for (int l = 0; l < a.layers; ++l) {
                uint4 rec = uint4{0u, 0u, 0u, 0u};
                if (hdr[l * 4 + 1]) rec.w = __float_as_uint(y[hdr[l * 4 + 2] + ldsp_wrap(r, hdr[l * 4 + 3], z)]);
                recs[(size_t)l * z] = rec;
            }
        }
        uint4 cur = uint4{0u, 0u, 0u, 0u};
        if (mine) cur = recs[0];
        lds_barrier();
        int time = 0, my_iters = a.max_iter;
        bool active = mine, clean = false;
        while (__ballot(active) != 0ull) {
            uint32_t last_bad = 0;
            for (int l = 0; l < a.layers; ++l) {
                const int ln = l + 1 < a.layers ? l + 1 : 0;
                uint4 nxt = uint4{0u, 0u, 0u, 0u};
                if (active && a.layers > 1) nxt = recs[(size_t)ln * z];
                const int dl = hdr[l * 4], ext = hdr[l * 4 + 1];
                const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                if (active) {
                    uint4 rec;
                    uint32_t par = 0;
                    bool done = false;
                    if (ext) {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D: done = ldsp_row<D, 1, false, true, CORR>(P, pk, z, r, cur, &rec, &par, corr); break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    } else {
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D + 1: done = ldsp_row<D + 1, 0, false, true, CORR>(P, pk, z, r, cur, &rec, &par, corr); break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                    }
                    if (!done) rec = ldsp_row_any<CORR>(P, pk, dl, ext, z, r, cur, zfs + (size_t)l * z, &par, corr);
                    last_bad = par;
                    asm volatile("" : "+v"(nxt.x), "+v"(nxt.y), "+v"(nxt.z), "+v"(nxt.w) : : "memory");
                    recs[(size_t)l * z] = rec;
                    if (a.layers == 1) nxt = rec;
                    if (ext) {
                        const uint64_t neg = __ballot(__uint_as_float(rec.w) < 0.0f);
                        const uint64_t act = __ballot(true);
                        if (lane == (int)__builtin_ctzll(act)) extneg[l] = neg;
                    }
                }
                lds_barrier();
                cur = nxt;
            }
            ++time;
            const bool check = a.early_term || time == a.rounds;
            const uint64_t last_mask = __ballot(active && last_bad);
            bool any_bad = true;
            if (check && __ballot(active && (last_mask & gmask) == 0ull) != 0ull) {
                /* some frame's last layer is all even: the full syndrome, for the frames that need it */
                uint64_t bad = 0;
                const bool need = active && (last_mask & gmask) == 0ull;
                if (need) {
                    for (int l = 0; l < a.layers; ++l) {
                        const int dl = hdr[l * 4], ext = hdr[l * 4 + 1];
                        const ldpc_const_i32 pk = pack + (size_t)l * kLdspPackStride;
                        uint64_t par = 0;
                        switch (dl) {
#define LDPC_LDSP_CASE(D) case D + 1: par = ldsp_row_parity<D + 1>(P, pk, z, r); break;
                            LDPC_LDSP_WIDTHS(LDPC_LDSP_CASE)
#undef LDPC_LDSP_CASE
                        default: break;
                        }
                        if (ext) par ^= extneg[l];
                        bad |= par;
                    }
                    any_bad = (bad & gmask) != 0ull;
                }
            }
            if (active) {
                clean = check && !any_bad;
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
                for (int bit = 0; bit < 8; ++bit) byte |= (P[j * 8 + bit] < 0.0f ? 1u : 0u) << bit;
                if (base + j < a.out_bytes) a.out[base + j] = (uint8_t)byte;
            }
            if (a.dump_p) {
                for (int bc = 0; bc < a.nb; ++bc) {
                    const int slot = cslot[bc];
                    if (slot >= 0) a.dump_p[(size_t)frame * a.N + bc * z + r] = P[slot * z + r];
                }
                for (int l = 0; l < a.layers; ++l)
                    if (hdr[l * 4 + 1])
                        a.dump_p[(size_t)frame * a.N + hdr[l * 4 + 2] + ldsp_wrap(r, hdr[l * 4 + 3], z)] =
                            __uint_as_float(recs[(size_t)l * z].w);
            }
            if (a.dump_r) {
                for (int l = 0; l < a.layers; ++l) {
                    const int d = hdr[l * 4] + hdr[l * 4 + 1], e0 = a.layer_e0[l];
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
        lds_barrier();                                             /* P is refilled for the next frames */
    }

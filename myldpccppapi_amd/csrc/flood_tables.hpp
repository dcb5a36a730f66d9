/*
 * flood_tables.hpp -- the kernel tables of the streaming flooding decoders, filled per arithmetic in
 * translation units of their own (flood_sp.hip, flood_ms*.hip, flood_msc*.hip, flood_bp*.hip) so that the library
 * builds in parallel: the flooding engine (engine_flood.hip) only sees function pointers.
 */
#pragma once

#include "flood_kernels.hpp"

namespace ldpc {

using CheckFn = void (*)(const CheckArgs);
using VarFn = void (*)(const VarArgs);
using LinkFn = void (*)(const CheckArgs, const LinkArgs);
/* group launches (several degree classes of a bucket in one launch: flood_check.hpp, flood_var.hpp) */
using CheckGroupFn = void (*)(const CheckArgs, const GroupClass *, int);
using VarGroupFn = void (*)(const VarArgs, const GroupClass *, int);
using InitFn = void (*)(const InitArgs);

constexpr int kVarBuckets = 3, kCheckBuckets = 4;
constexpr int kVarBucketLo[kVarBuckets] = {1, 5, 9}, kVarBucketHi[kVarBuckets] = {4, 8, 16};
constexpr int kCheckBucketLo[kCheckBuckets] = {1, 9, 17, 25}, kCheckBucketHi[kCheckBuckets] = {8, 16, 24, 32};

struct FloodFns {
    CheckFn check[kMaxUnrolledCheckDegreeMS + 1] = {};        /* narrow waves (1 value per lane) */
    CheckFn check_wide[kMaxUnrolledCheckDegreeMS + 1] = {};   /* V values per lane */
    LinkFn link[kMaxUnrolledDegree + 1] = {};                 /* wide waves */
    LinkFn link_narrow[kMaxUnrolledDegree + 1] = {};          /* narrow waves */
    LinkFn link_deep[kMaxUnrolledDegree + 1] = {};            /* narrow waves, inputs two rows ahead */
    LinkFn link_half[kMaxUnrolledDegree + 1] = {};            /* 2 values per lane (V = 4) */
    VarFn var[kMaxUnrolledDegree + 1] = {};
    CheckGroupFn check_group[kCheckBuckets] = {};
    int check_group_width = 1;                                /* values per lane of the group check kernels */
    VarGroupFn var_group[kVarBuckets] = {};
    InitFn init = nullptr;
    InitFn init_in[3] = {};                                   /* by enum ldpc_llr_type: [0] = init (float), fp16, int8 input */
    int max_check_unrolled = kMaxUnrolledDegree;
};

/* V = frames per lane (1, 2 or 4) */
void fill_flood_sp(int V, FloodFns *f);      /* sum-product, fp32            (flood_sp.hip)   */
void fill_flood_ms(int V, FloodFns *f);      /* min-sum, fp32 messages       (flood_ms.hip)   */
void fill_flood_ms16(int V, FloodFns *f);    /* min-sum, fp16 message storage (flood_ms16.hip) */
void fill_flood_msc(int V, FloodFns *f);     /* corrected min-sum (kAlgoMSC), fp32 messages (flood_msc.hip)   */
void fill_flood_msc16(int V, FloodFns *f);   /* corrected min-sum, fp16 message storage     (flood_msc16.hip) */
void fill_flood_ms8(int V, FloodFns *f);     /* min-sum, fp8 (E4M3) message storage         (flood_ms8.hip)   */
void fill_flood_msc8(int V, FloodFns *f);    /* corrected min-sum, fp8 message storage      (flood_msc8.hip)  */
void fill_flood_msi4(int V, FloodFns *f);    /* min-sum, 4-bit fixed-point message storage (flood_msi4.hip)   */
void fill_flood_msci4(int V, FloodFns *f);   /* corrected min-sum, 4-bit fixed point        (flood_msci4.hip)  */
void fill_flood_msi5(int V, FloodFns *f);    /* min-sum, 5-bit fixed-point message storage (flood_msi5.hip)   */
void fill_flood_msci5(int V, FloodFns *f);   /* corrected min-sum, 5-bit fixed point        (flood_msci5.hip)  */
void fill_flood_msi6(int V, FloodFns *f);    /* min-sum, 6-bit fixed-point message storage (flood_msi6.hip)   */
void fill_flood_msci6(int V, FloodFns *f);   /* corrected min-sum, 6-bit fixed point        (flood_msci6.hip)  */
void fill_flood_msi8(int V, FloodFns *f);    /* min-sum, 8-bit fixed-point message storage (flood_msi8.hip)   */
void fill_flood_msci8(int V, FloodFns *f);   /* corrected min-sum, 8-bit fixed point        (flood_msci8.hip)  */
void fill_flood_bp(int V, FloodFns *f);      /* log-domain sum-product (kAlgoBP), fp32 messages (flood_bp.hip)  */
void fill_flood_bp16(int V, FloodFns *f);    /* log-domain sum-product, fp16 message storage    (flood_bp16.hip) */

}  // namespace ldpc

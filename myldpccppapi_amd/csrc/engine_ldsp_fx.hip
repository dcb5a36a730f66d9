/* engine_ldsp_fx.hip -- the fixed-point record kernel (ldsp_fx_kernels.hpp): int16 posteriors in LDS, 8-byte check records
 * in cache. */
#define LDPC_ENGINE_LDSP_FX
#include "ldsp_fx_kernels.hpp"
#include "engines.hpp"
namespace ldpc {
hipError_t engine_ldsp_fx_plan_create(LdspPlan *pl, int32_t M, int32_t N, int64_t E, const std::vector<int32_t> &row_ptr,
                                      const std::vector<int32_t> &cols, int32_t z, int32_t K, int64_t max_batch, int device,
                                      const Tune &tune)
{
    return ldsp_fx_plan_create(pl, M, N, E, row_ptr, cols, z, K, max_batch, device, tune);
}
hipError_t engine_ldsp_fx_run(LdspPlan *pl, const FusedRun &r, hipStream_t s, int32_t *launched) { return ldsp_fx_run(pl, r, s, launched); }
}  // namespace ldpc

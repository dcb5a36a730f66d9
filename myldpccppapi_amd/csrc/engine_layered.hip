/* engine_layered.hip -- the streaming layered engine on float P and R, one launch per layer (layered_kernels.hpp), and the
 * engine's entry point. */
#define LDPC_ENGINE_LAYERED
#include "layered_kernels.hpp"
#include "engines.hpp"
namespace ldpc {
hipError_t engine_layered_fx_run(LayeredPlan *pl, const LayeredRun &r, hipStream_t s, int32_t *launched);   /* engine_layered_fx.hip */
hipError_t engine_layered_run(LayeredPlan *pl, const LayeredRun &r, hipStream_t s, int32_t *launched)
{
    return pl->fixed() ? engine_layered_fx_run(pl, r, s, launched) : layered_run<StoreF32>(pl, r, s, launched);
}
}  // namespace ldpc

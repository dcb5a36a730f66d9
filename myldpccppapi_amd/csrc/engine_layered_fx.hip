/* engine_layered_fx.hip -- the streaming layered engine on one-byte R and int16 P (LDPC_ALGO_LAYERED_FX, kLayerFx in
 * layered_kernels.hpp), a unit of its own so that it builds beside engine_layered.hip, which forwards to it. */
#define LDPC_ENGINE_LAYERED
#include "layered_kernels.hpp"
namespace ldpc {
hipError_t engine_layered_fx_run(LayeredPlan *pl, const LayeredRun &r, hipStream_t s, int32_t *launched) { return layered_run<StoreFx>(pl, r, s, launched); }
}  // namespace ldpc

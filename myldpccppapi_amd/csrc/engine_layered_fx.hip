/* engine_layered_fx.hip -- the fixed-point rule of the streaming layered engine (LDPC_ALGO_LAYERED_FX, kLayerFx in
 * layered_kernels.hpp): one-byte R, int16 P, one launch per layer. */
#define LDPC_ENGINE_LAYERED_FX
#include "layered_kernels.hpp"
#include "engines.hpp"
namespace ldpc {
hipError_t engine_layered_fx_run(LayeredPlan *pl, const LayeredRun &r, hipStream_t s, int32_t *launched) { return layered_fx_run(pl, r, s, launched); }
}  // namespace ldpc

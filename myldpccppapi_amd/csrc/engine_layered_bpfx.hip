/* engine_layered_bpfx.hip -- the kernels of LDPC_ALGO_LAYERED_BP_FX (kLayerBpFx in layered_kernels.hpp): box-plus rows in
 * fixed point on one-byte R and int16 P.  A unit of its own so that its 75 kernels build beside engine_layered.hip and
 * engine_layered_fx.hip; the driver that launches them is the instantiation on StoreFx in engine_layered_fx.hip, which
 * takes them as a table. */
#define LDPC_ENGINE_LAYERED
#include "layered_kernels.hpp"
namespace ldpc {
void layer_table_bpfx(int V, LayerFn<StoreFx> *t)
{
    const std::make_integer_sequence<int, kMaxUnrolledLayerDegree> degrees;
    if (V == 1) layer_table_fill<1, kLayerBpFx>(t, degrees);
    else if (V == 2) layer_table_fill<2, kLayerBpFx>(t, degrees);
    else layer_table_fill<4, kLayerBpFx>(t, degrees);
}
}  // namespace ldpc

/* engine_bitflip.hip -- the hard-decision bit-flipping engine (LDPC_ALGO_BITFLIP, bitflip_kernels.hpp): its kernels and the
 * driver that launches them, a unit of its own so that it builds beside the other engines. */
#define LDPC_ENGINE_BITFLIP
#include "layered_kernels.hpp"
#include "bitflip_kernels.hpp"
namespace ldpc {
hipError_t engine_bitflip_run(BitflipPlan *pl, const BitflipRun &r, hipStream_t s, int32_t *launched) { return bitflip_run(pl, r, s, launched); }
}  // namespace ldpc

/* flood_msi8.hip -- min-sum with 8-bit fixed-point message storage (LDPC_MSG_I8, msg_bits = 8: integers in [-127, 127]): instantiations of the streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_msi8(int V, FloodFns *f) { tables::fill<kAlgoMS, q8<127>>(V, f); } }

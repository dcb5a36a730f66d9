/* flood_msi5.hip -- min-sum with 5-bit fixed-point message storage (LDPC_MSG_I8, msg_bits = 5: integers in [-15, 15]): instantiations of the streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_msi5(int V, FloodFns *f) { tables::fill<kAlgoMS, q8<15>>(V, f); } }

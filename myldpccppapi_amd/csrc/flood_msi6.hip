/* flood_msi6.hip -- min-sum with 6-bit fixed-point message storage (LDPC_MSG_I8, msg_bits = 6: integers in [-31, 31]): instantiations of the streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_msi6(int V, FloodFns *f) { tables::fill<kAlgoMS, q8<31>>(V, f); } }

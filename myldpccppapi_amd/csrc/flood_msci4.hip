/* flood_msci4.hip -- corrected min-sum with 4-bit fixed-point message storage (LDPC_MSG_I8, msg_bits = 4: integers in [-7, 7]): instantiations of the streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_msci4(int V, FloodFns *f) { tables::fill<kAlgoMSC, q8<7>>(V, f); } }

/* flood_ms8.hip -- min-sum with fp8 (E4M3) message storage: instantiations of the streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_ms8(int V, FloodFns *f) { tables::fill<kAlgoMS, f8>(V, f); } }

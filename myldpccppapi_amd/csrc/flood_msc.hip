/* flood_msc.hip -- normalized / offset min-sum (fp32 messages) instantiations of the streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_msc(int V, FloodFns *f) { tables::fill<kAlgoMSC, float>(V, f); } }

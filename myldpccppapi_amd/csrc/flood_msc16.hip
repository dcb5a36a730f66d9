/* flood_msc16.hip -- normalized / offset min-sum with fp16 message storage: streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_msc16(int V, FloodFns *f) { tables::fill<kAlgoMSC, hf>(V, f); } }

/* flood_bp16.hip -- log-domain sum-product (box-plus check node) with fp16 message storage: streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_bp16(int V, FloodFns *f) { tables::fill<kAlgoBP, hf>(V, f); } }

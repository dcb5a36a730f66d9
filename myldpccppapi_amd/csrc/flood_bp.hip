/* flood_bp.hip -- log-domain sum-product (box-plus check node), fp32 messages: streaming flooding kernels. */
#include "flood_tables_impl.hpp"
namespace ldpc { void fill_flood_bp(int V, FloodFns *f) { tables::fill<kAlgoBP, float>(V, f); } }

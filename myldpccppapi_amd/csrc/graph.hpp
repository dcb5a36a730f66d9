/*
 * graph.hpp -- the graph behind an `ldpc_graph *`, shared by the decoder driver and encoder.hip.
 */
#pragma once

#include <stdint.h>

#include <vector>

struct ldpc_graph {
    int32_t M = 0, N = 0;
    int64_t E = 0;
    std::vector<int32_t> rows, cols;        /* [E] hRows, hCols           */
    std::vector<int32_t> row_ptr;           /* [M+1] hRowRange            */
    std::vector<int32_t> col_ptr, col_edge; /* CSC, edges ascending       */
    int32_t max_row_deg = 0, max_col_deg = 0;
};

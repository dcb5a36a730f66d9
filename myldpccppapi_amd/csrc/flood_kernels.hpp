/*
 * flood_kernels.hpp -- gfx950 kernels for two-phase (flooding) LDPC belief
 * propagation: sum-product in the probability domain and min-sum, fp32.
 *
 * Replaces the reference's kernel chain (decodeCL.c):
 *   check_kernel<SP>  <- refreshR        decodeCL.c:25-41
 *   var_kernel<SP>    <- hardDecision    decodeCL.c:64-86  + refreshQ :43-62
 *   check_kernel<MS>  <- refreshRMS      decodeCL.c:126-147
 *   syndrome_kernel   <- checkResult     decodeCL.c:88-108
 *   var_kernel<MS>    <- refreshPostPMS  decodeCL.c:149-171 + refreshQMS :175-186
 *   init_kernel       <- decodeInit :3-22 / decodeInitMS :113-124
 *   pack_kernel       <- toChar :188-199 (and decodeCPU's bit packing MyLdpc.cpp:765-774)
 *
 * Design (MI355X-first, not the reference's layout):
 *   - The reference indexes messages [frame][edge] with the frame as NDRange
 *     dim 0, so adjacent work-items are E floats apart, and every edge re-walks
 *     its whole row/column (O(d^2) reads).  Here FRAMES ARE THE LANES: a tile is
 *     F = 64*V frames (V = 1, 2 or 4 frames per lane) and every per-edge message
 *     of a tile is one contiguous F*4-byte segment, msg[tile][edge][F].  A
 *     wave-instruction moves one whole segment (256 B .. 1 KiB, 16 B per lane at
 *     V = 4), H's indices are wave-uniform (scalar loads, SGPRs), each message is
 *     read once and written once per half-iteration, and the check / variable
 *     reductions are per-lane register chains -- no cross-lane traffic, no LDS,
 *     no MFMA (sparse gather/reduce, HBM-bound).
 *   - Check phase: a row's edges are consecutive edge ids, so it streams.
 *     Variable phase: a column's edges are gathered/scattered as whole segments.
 *   - fp32 results are bit-identical to the reference's operation order:
 *     products/sums run left to right in ascending edge id with the own edge
 *     skipped (prefix shared, tail recomputed), IEEE division, no FMA
 *     contraction (compile with -ffp-contract=off).
 *   - SP messages are stored as ONE float per edge and direction: the reference
 *     only ever consumes q0-q1 (decodeCL.c:37) and r0 = (1+d)/2, r1 = (1-d)/2 are
 *     exact functions of d (:39-40), so storing d_q = fl(q0-q1) and d_r = d loses
 *     nothing: 16*E + 4*N bytes per frame-iteration.
 *   - Hard bits live as bit masks hard[tile][n][V] (bit l of word v = frame
 *     V*l+v): the row syndrome is an XOR of wave-uniform 64-bit words.
 */
#pragma once

/* The kernels by role; this file is the umbrella include.
 *   flood_common.hpp    stream loads and stores, tile selection, CheckArgs / VarArgs / GroupClass, Q slots, MsCorr
 *   flood_check.hpp     check_sp / check_ms / check_bp / check_node, check_rows, check_kernel, generic, group
 *   flood_var.hpp       var_sp, var_columns, var_kernel, group, generic
 *   flood_link.hpp      the column-fused check kernels: wide, narrow / half, deep
 *   flood_round.hpp     init, syndrome, state, pack
 *   flood_handover.hpp  compact_*, tail_* */
#include "flood_common.hpp"
#include "flood_check.hpp"
#include "flood_var.hpp"
#include "flood_link.hpp"
#include "flood_round.hpp"
#include "flood_handover.hpp"

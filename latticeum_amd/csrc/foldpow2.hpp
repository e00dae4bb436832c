// foldpow2.hpp -- the index arithmetic of the coefficient-form fold at d = 16 .. 512
// (fold_coeff_pow2.hip): the reversed byte table of a challenge, the 16 table bytes a
// lane cuts from it as its share of an A tile, the 16 packed words that hold a lane's
// share of a B tile, and the split of an element tile's rows over waves. Plain integer
// code that also compiles for the host alone (tests/test_fold_pow2_host.py runs it under
// the address and UB sanitizers; tests/test_fold_pow2_model.py restates it in numpy).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "digitpack.hpp"

namespace lfk {

constexpr int FP2_MAXW = 30;  // 2K <= 30

// The table of one challenge rho (coefficients in [-127, 127]) at degree d: with the
// signed generator g[delta] = rho[delta] (delta >= 0), -rho[delta + d] (delta < 0) of
// the negacyclic Toeplitz matrix R[c][j] = g[c - j],
//   tab[d - delta] = g[delta], -d < delta < d;  tab[0] = 0;  tab[2d .. 2d + 31] = 0.
// Reversed, so that the bytes of a row of R at increasing j lie at increasing addresses.
LF_HD int fp2_tab_bytes(int d) { return 2 * d + 32; }
LF_HD int fp2_tab_pos(int d, int delta) { return d - delta; }
// the one or two positions coefficient c of rho is written to, and its sign there
LF_HD int fp2_tab_pos_plus(int d, int c) { return d - c; }       // g[c] = rho[c]
LF_HD int fp2_tab_pos_minus(int d, int c) { return 2 * d - c; }  // g[c - d] = -rho[c], c > 0

// An element tile is 32 elements (the columns of a 32 x 32 x 32 product); its d rows are
// d / 32 row tiles, of which a wave owns fp2_rows_per_wave (up to 8: 128 accumulator
// registers); fp2_waves_per_tile waves share the tile and a block of four waves holds
// fp2_tiles_per_block element tiles. d = 16: one row tile whose rows 16 .. 31 are zero.
LF_HD int fp2_row_tiles(int d) { return d >= 32 ? d / 32 : 1; }
LF_HD int fp2_rows_per_wave(int d) { return fp2_row_tiles(d) < 8 ? fp2_row_tiles(d) : 8; }
LF_HD int fp2_waves_per_tile(int d) { return fp2_row_tiles(d) / fp2_rows_per_wave(d); }
LF_HD int fp2_tiles_per_block(int d) { return 4 / fp2_waves_per_tile(d); }

// d >= 32. Lane l = col + 32 h of a wave holds A[row col][k = 16 h + x] and
// B[k = 16 h + x][column col], x < 16 (v_mfma_i32_32x32x32_i8). In the product of row
// tile t and column tile q, row = 32 t + col and j = 32 q + 16 h + x, so the lane's A
// bytes are g[32 (t - q) + col - 16 h - x] = tab[o + x] with
LF_HD int fp2_a_offset(int d, int lane, int t, int q) { return d + 16 * (lane >> 5) - (lane & 31) - 32 * (t - q); }
// and its B bytes are digits of the coefficients j = 32 q + 16 h + x of element col: the
// half fp2_b_half of the 16 consecutive words from fp2_b_word on (digitpack.hpp smp2).
LF_HD int fp2_b_word(int d, int lane, int q) { return (32 * q + 16 * (lane >> 5)) & (d / 2 - 1); }
LF_HD int fp2_b_half(int d, int lane, int q) { return smp2_half_of(d, 32 * q + 16 * (lane >> 5)); }

// d = 16. One product holds two witnesses: lane half h takes witness 2 m + h, its k
// index x < 16 is the coefficient j = x, rows 16 .. 31 of A are zero. A bytes:
// g[col - x] = tab[o + x], o = 16 - col (col < 16); B: words 0 .. 7 of the element, the
// low halves (j < 8) then the high ones.
LF_HD int fp2_a_offset16(int lane) { return 16 - (lane & 15); }

// The accumulator register i < 16 of lane l holds row 8 (i / 4) + 4 h + (i % 4) of the tile
LF_HD int fp2_acc_row(int lane, int i) { return 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3); }

// the digit byte of a sign|magnitude half word at plane k: 0x00, 0x01 or 0xFF
LF_HD uint32_t fp2_digit_byte(uint32_t hw, int k) { return (uint32_t)(uint8_t)(int8_t)sm16_digit(hw, k); }

// witness units [u0, u1) of split ks of ks_n (a unit is one witness; d = 16 does not split)
LF_HD int fp2_split_begin(int nw, int ks, int ks_n) { return ks * nw / ks_n; }

}  // namespace lfk

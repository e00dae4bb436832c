// witness_wire.hpp -- the witness wire format's header and sizes (lf.h, "witness wire
// format"). Host code with no dependency but lf.h, so a stand-alone program can
// drive the parser; witness_wire.cpp exports it, api_witness.hip reads and writes the
// payload behind it.
//   bytes 0-3 "LFW1" | 4-7 u32 d | 8-11 u32 L | 12-15 u32 bits | 16-23 u64 N | 24-31 u64 0
//   then N d integers of `bits` bits, little-endian, coefficient c of element e at e d + c
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/lf.h"

namespace lfk {

constexpr size_t WIRE_HEADER = 32;

// the rings of the library: Phi_72 and X^d + 1 for d = 16 .. 4096 (launch.hpp NegaDegrees)
inline bool wire_ring_ok(int d) { return d == 24 || (d >= 16 && d <= 4096 && (d & (d - 1)) == 0); }
inline bool wire_bits_ok(int bits) { return bits == 16 || bits == 32 || bits == 64; }

// N d bits / 8, or false when it (or the header on top of it) does not fit size_t
inline bool wire_payload_len(uint64_t d, uint64_t N, uint64_t bits, size_t *out) {
  const uint64_t per = d * (bits / 8);  // <= 4096 * 8
  if (per && N > (SIZE_MAX - WIRE_HEADER) / per) return false;
  *out = (size_t)(N * per);
  return true;
}

inline uint64_t wire_le(const uint8_t *p, int n) {
  uint64_t v = 0;
  for (int i = 0; i < n; i++) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
inline void wire_put_le(uint8_t *p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) p[i] = (uint8_t)(v >> (8 * i));
}

inline void wire_write_header(uint8_t *out, int d, int L, int bits, uint64_t N) {
  out[0] = 'L', out[1] = 'F', out[2] = 'W', out[3] = '1';
  wire_put_le(out + 4, (uint32_t)d, 4);
  wire_put_le(out + 8, (uint32_t)L, 4);
  wire_put_le(out + 12, (uint32_t)bits, 4);
  wire_put_le(out + 16, N, 8);
  wire_put_le(out + 24, 0, 8);
}

// every format check of the deserializer; reads in[0 .. min(len, 32)) only
inline int wire_parse_header(const uint8_t *in, size_t len, int *d, int *L, int *bits, size_t *N) {
  if (!in) return LF_ERR_INVALID_ARG;
  if (len < WIRE_HEADER) return LF_ERR_INCORRECT_LENGTH;
  if (in[0] != 'L' || in[1] != 'F' || in[2] != 'W' || in[3] != '1') return LF_ERR_INVALID_ARG;
  const uint64_t hd = wire_le(in + 4, 4), hL = wire_le(in + 8, 4), hb = wire_le(in + 12, 4);
  const uint64_t hN = wire_le(in + 16, 8), rsv = wire_le(in + 24, 8);
  if (hd > 4096 || !wire_ring_ok((int)hd)) return LF_ERR_UNSUPPORTED_RING;
  if (!wire_bits_ok(hb > 64 ? 0 : (int)hb) || rsv != 0 || hL < 1 || hL > INT32_MAX || hN % hL) return LF_ERR_INVALID_ARG;
  size_t pay;
  if (hN > SIZE_MAX || !wire_payload_len(hd, hN, hb, &pay) || len != WIRE_HEADER + pay) return LF_ERR_INCORRECT_LENGTH;
  if (d) *d = (int)hd;
  if (L) *L = (int)hL;
  if (bits) *bits = (int)hb;
  if (N) *N = (size_t)hN;
  return LF_OK;
}

}  // namespace lfk

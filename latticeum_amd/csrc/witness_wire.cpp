// witness_wire.cpp -- the host-only entries of the witness wire format: the payload
// size and the header parser (witness_wire.hpp). No context, no device work.
#include "witness_wire.hpp"

extern "C" {

size_t lf_witness_packed_len(int d, size_t N, int bits) {
  size_t n;
  if (!lfk::wire_ring_ok(d) || !lfk::wire_bits_ok(bits) || !lfk::wire_payload_len((uint64_t)d, N, (uint64_t)bits, &n))
    return 0;
  return n;
}

int lf_witness_wire_header(const uint8_t *in, size_t len, int *d, int *L, int *bits, size_t *N) {
  return lfk::wire_parse_header(in, len, d, L, bits, N);
}

}  // extern "C"

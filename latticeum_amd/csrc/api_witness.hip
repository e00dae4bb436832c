// api_witness.hip -- Witness::from_f_coeff (LF/arith.rs:324-338) as a public entry at
// every ring, and the packed witness: the width probe, pack / unpack on the device,
// and the wire bytes (lf.h, "witness wire format"; the header and its checks are
// witness_wire.hpp's). The kernels are witness_pack.hip's and, for plain u64 words at
// d = 1024, kernels_n32.hip's k_from_fcoeff_n32 and its split form.
#include "api_internal.hpp"
#include "witness_wire.hpp"
#include "wsrc.hpp"

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the payload source of a width (a u64 payload word is checked against p)
int payload_src(int bits) {
  return bits == 16 ? lfk::WSRC_I16 : bits == 32 ? lfk::WSRC_I32 : lfk::WSRC_U64_CHECKED;
}

}  // namespace

extern "C" {

int lf_dev_witness_from_f_coeff(lf_ctx *c, const lf_params *pr, const uint64_t *fc, size_t N, uint64_t *f,
                                uint64_t *w) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  if (N && (!fc || !f || !w)) return fail(c, LF_ERR_INVALID_ARG, "from_f_coeff: null buffer");
  if (!aligned16(fc) || !aligned16(f) || !aligned16(w))
    return fail(c, LF_ERR_INVALID_ARG, "from_f_coeff: the buffers must be 16-byte aligned");
  Tables *t;
  LF_TRY(get_tables(c, pr->d, t));
  LF_HIP(c, lfk::from_fcoeff(fc, lfk::WSRC_U64, N, pr->d, lb, pr->L, nullptr, f, w, t->fwd, c->d_err, c->cur));
  return LF_OK;
}

int lf_witness_from_f_coeff(lf_ctx *c, const lf_params *pr, const uint64_t *fc, size_t N, uint64_t *f, uint64_t *w,
                            int repr) {
  DevGuard g(c);
  if (!c || (!fc && N) || !f || !w) return LF_ERR_INVALID_ARG;
  LF_TRY(check_repr(c, repr));
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  const int d = pr->d;
  DevBuf dfc, df, dw;
  LF_TRY(upload(c, dfc, fc, N * d, repr));
  LF_TRY(dev_alloc(c, df, N * d));
  LF_TRY(dev_alloc(c, dw, N / pr->L * d));
  LF_TRY(lf_dev_witness_from_f_coeff(c, pr, dfc.p, N, df.p, dw.p));
  LF_TRY(download(c, f, df, N * d, repr));
  LF_TRY(download(c, w, dw, N / pr->L * d, repr));
  return lf_ctx_sync(c);
}

int lf_dev_witness_bits(lf_ctx *c, int d, const uint64_t *fc, size_t N, int *bits, uint64_t *norm) {
  DevGuard g(c);
  if (!c || !bits || !norm || (N && !fc)) return LF_ERR_INVALID_ARG;
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  if ((uintptr_t)fc & 7) return fail(c, LF_ERR_INVALID_ARG, "witness bits: the words must be 8-byte aligned");
  const size_t n = N * (size_t)d;
  LF_TRY(grow(c, c->rel, c->rel_elems, (size_t)4));
  LF_HIP(c, lfk::linf_norm(fc, n, c->rel, c->cur));
  LF_HIP(c, lfk::witness_range(fc, n, c->rel + 2, c->cur));
  uint64_t h[4];
  LF_HIP(c, hipMemcpyAsync(h, c->rel, sizeof h, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  *norm = h[0];
  *bits = h[3] ? 64 : h[2] ? 32 : 16;
  return LF_OK;
}

int lf_dev_witness_pack(lf_ctx *c, int d, const uint64_t *fc, size_t N, int bits, void *packed) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  if (!ring_ok(d)) return fail(c, LF_ERR_UNSUPPORTED_RING, "unsupported ring degree");
  if (!lfk::wire_bits_ok(bits)) return fail(c, LF_ERR_INVALID_ARG, "witness pack: bits must be 16, 32 or 64");
  if (N && (!fc || !packed)) return fail(c, LF_ERR_INVALID_ARG, "witness pack: null buffer");
  if (!aligned16(fc) || !aligned16(packed))
    return fail(c, LF_ERR_INVALID_ARG, "witness pack: the buffers must be 16-byte aligned");
  LF_HIP(c, lfk::witness_pack(fc, N * (size_t)d, bits, packed, c->d_err, c->cur));
  return LF_OK;
}

int lf_dev_witness_unpack(lf_ctx *c, const lf_params *pr, const void *packed, int bits, size_t N, uint64_t *fc,
                          uint64_t *f, uint64_t *w) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (!lfk::wire_bits_ok(bits)) return fail(c, LF_ERR_INVALID_ARG, "witness unpack: bits must be 16, 32 or 64");
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  if (!f != !w) return fail(c, LF_ERR_INVALID_ARG, "witness unpack: f and w_ccs come together or not at all");
  if (N && (!packed || !fc)) return fail(c, LF_ERR_INVALID_ARG, "witness unpack: null buffer");
  if (!aligned16(packed) || !aligned16(fc) || !aligned16(f) || !aligned16(w))
    return fail(c, LF_ERR_INVALID_ARG, "witness unpack: the buffers must be 16-byte aligned");
  const int d = pr->d;
  if (!f) {
    LF_HIP(c, lfk::witness_decode(packed, payload_src(bits), N * (size_t)d, fc, c->d_err, c->cur));
    return LF_OK;
  }
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  LF_HIP(c, lfk::from_fcoeff(packed, payload_src(bits), N, d, lb, pr->L, fc, f, w, t->fwd, c->d_err, c->cur));
  return LF_OK;
}

int lf_witness_serialize(lf_ctx *c, const lf_params *pr, const lf_witness *w, size_t N, int bits, uint8_t *out,
                         size_t cap, size_t *len) {
  DevGuard g(c);
  if (!c || !len) return LF_ERR_INVALID_ARG;
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (!w || (N && !w->f_coeff)) return fail(c, LF_ERR_INVALID_ARG, "witness serialize: null witness");
  if (bits != 0 && !lfk::wire_bits_ok(bits))
    return fail(c, LF_ERR_INVALID_ARG, "witness serialize: bits must be 0, 16, 32 or 64");
  if (N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a multiple of L");
  const int d = pr->d;
  if (bits == 0) {  // the narrowest width: one canonical encoding per witness
    uint64_t norm;
    LF_TRY(lf_dev_witness_bits(c, d, w->f_coeff, N, &bits, &norm));
  }
  size_t pay;
  if (!lfk::wire_payload_len((uint64_t)d, N, (uint64_t)bits, &pay))
    return fail(c, LF_ERR_INVALID_ARG, "witness serialize: the size does not fit size_t");
  *len = lfk::WIRE_HEADER + pay;
  if (!out || cap < *len) return LF_ERR_INCORRECT_LENGTH;
  DevBuf dp;
  LF_TRY(dev_alloc(c, dp, (pay + 7) / 8));
  LF_TRY(lf_dev_witness_pack(c, d, w->f_coeff, N, bits, dp.p));
  if (pay) LF_HIP(c, hipMemcpyAsync(out + lfk::WIRE_HEADER, dp.p, pay, hipMemcpyDeviceToHost, c->cur));
  lfk::wire_write_header(out, d, pr->L, bits, N);
  return lf_ctx_sync(c);  // LF_ERR_DECOMPOSITION_OVERFLOW: a coefficient does not fit the width asked for
}

int lf_witness_deserialize(lf_ctx *c, const lf_params *pr, const uint8_t *in, size_t len, const lf_witness *out,
                           size_t N) {
  DevGuard g(c);
  if (!c) return LF_ERR_INVALID_ARG;
  int hd, hL, bits;
  size_t hN;
  const int rc = lfk::wire_parse_header(in, len, &hd, &hL, &bits, &hN);
  if (rc != LF_OK) return fail(c, rc, "witness deserialize: malformed header or length");
  int lb, lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (hd != pr->d || hL != pr->L) return fail(c, LF_ERR_INVALID_ARG, "witness deserialize: d or L differ from the params");
  if (hN != N) return fail(c, LF_ERR_INVALID_ARG, "witness deserialize: N differs from the bytes' N");
  if (!out || (N && (!out->f_coeff || !out->f || !out->w_ccs)))
    return fail(c, LF_ERR_INVALID_ARG, "witness deserialize: null witness buffer");
  const size_t pay = len - lfk::WIRE_HEADER;
  DevBuf dp;
  LF_TRY(dev_alloc(c, dp, (pay + 7) / 8));
  if (pay) LF_HIP(c, hipMemcpyAsync(dp.p, in + lfk::WIRE_HEADER, pay, hipMemcpyHostToDevice, c->cur));
  LF_TRY(lf_dev_witness_unpack(c, pr, dp.p, bits, N, out->f_coeff, out->f, out->w_ccs));
  const int rs = lf_ctx_sync(c);
  if (rs == LF_ERR_DECOMPOSITION_OVERFLOW)  // the unpack kernel's flag: a 64-bit word >= p
    return fail(c, LF_ERR_INVALID_ARG, "witness deserialize: a payload word is not a canonical residue");
  return rs;
}

}  // extern "C"

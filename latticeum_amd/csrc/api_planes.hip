// api_planes.hip -- the way into and out of the packed digit planes without a step
// (lf.h, lf_fold_step_bufs.planes): lf_dev_pack_planes (f_coeff -> planes), lf_dev_planes_witness
// (planes -> f_coeff, f, w_ccs) and lf_dev_planes_check (the l_inf norm, and whether a packer
// wrote the bytes). The kernels are planes_witness.hip's, kernels_n32.hip's k_pack_sm and
// kernels_n4k.hip's k_pack_sm8, and witness_pack.hip's from_fcoeff. None of the three reads or
// writes the step state, the operand rows or the dead flags.
#include "api_internal.hpp"
#include "wsrc.hpp"

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// pr names a packed form of a supported ring, and N is a positive multiple of L
int planes_args(lf_ctx *c, const lf_params *pr, size_t N, int &lb) {
  if (!pr) return fail(c, LF_ERR_INVALID_ARG, "null params");
  if (!lf_fold_step_planes_len(pr, 1))
    return fail(c, LF_ERR_UNSUPPORTED_RING, "packed planes: d = 24, 16 .. 512, 1024 or 4096, b_small = 2, K <= 15");
  int lbs;
  LF_TRY(check_params(c, pr, lb, lbs));
  if (!N || N % pr->L) return fail(c, LF_ERR_INCORRECT_LENGTH, "N must be a positive multiple of L");
  return LF_OK;
}

}  // namespace

extern "C" {

int lf_dev_pack_planes(lf_ctx *c, const lf_params *pr, const uint64_t *fc, size_t N, uint64_t *planes) {
  if (!c) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!pr || !fc || !planes) return fail(c, LF_ERR_INVALID_ARG, "pack_planes: NULL pointer");
  int lb;
  LF_TRY(planes_args(c, pr, N, lb));
  if (!aligned16(fc) || !aligned16(planes))
    return fail(c, LF_ERR_INVALID_ARG, "pack_planes: the buffers must be 16-byte aligned");
  LF_HIP(c, lfk::planes_pack(fc, N, pr->d, pr->K, planes, c->d_err, c->cur));
  return LF_OK;
}

int lf_dev_planes_witness(lf_ctx *c, const lf_params *pr, const uint64_t *planes, size_t N, uint64_t *fc, uint64_t *f,
                          uint64_t *w) {
  if (!c) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!pr || !planes) return fail(c, LF_ERR_INVALID_ARG, "planes_witness: NULL pointer");
  if (!fc && !f && !w) return fail(c, LF_ERR_INVALID_ARG, "planes_witness: no output");
  int lb;
  LF_TRY(planes_args(c, pr, N, lb));
  if (!aligned16(planes) || !aligned16(fc) || !aligned16(f) || !aligned16(w))
    return fail(c, LF_ERR_INVALID_ARG, "planes_witness: the buffers must be 16-byte aligned");
  const int d = pr->d;
  const size_t n = N * (size_t)d;
  // from_fcoeff reads a canonical f_coeff and writes f and w_ccs together: an output the caller
  // does not take goes to the context's scratch ([N][d] words each, never [K][N][d])
  const bool crt = f || w;
  const size_t need = (fc ? 0 : n) + (crt && !f ? n : 0) + (crt && !w ? n / pr->L : 0);
  if (crt && need) LF_TRY(grow(c, c->pwit, c->pwit_elems, need));
  uint64_t *tmp = c->pwit;
  if (crt && !fc) fc = tmp, tmp += n;
  if (crt && !f) f = tmp, tmp += n;
  if (crt && !w) w = tmp;
  LF_HIP(c, lfk::planes_recompose(planes, N, d, pr->K, fc, c->cur));
  if (!crt) return LF_OK;
  Tables *t;
  LF_TRY(get_tables(c, d, t));
  LF_HIP(c, lfk::from_fcoeff(fc, lfk::WSRC_U64, N, d, lb, pr->L, nullptr, f, w, t->fwd, c->d_err, c->cur));
  return LF_OK;
}

int lf_dev_planes_check(lf_ctx *c, const lf_params *pr, const uint64_t *planes, size_t N, uint64_t bound,
                        uint64_t *norm, int *fault, size_t *where) {
  if (!c) return LF_ERR_INVALID_ARG;
  DevGuard g(c);
  if (!pr || !planes || !norm || !fault || !where) return fail(c, LF_ERR_INVALID_ARG, "planes_check: NULL pointer");
  int lb;
  LF_TRY(planes_args(c, pr, N, lb));
  if (!aligned16(planes)) return fail(c, LF_ERR_INVALID_ARG, "planes_check: the planes must be 16-byte aligned");
  LF_TRY(grow(c, c->rel, c->rel_elems, (size_t)4));
  LF_HIP(c, lfk::planes_scan(planes, N, pr->d, pr->K, bound, c->rel, c->cur));
  uint64_t h[3];
  LF_HIP(c, hipMemcpyAsync(h, c->rel, sizeof h, hipMemcpyDeviceToHost, c->cur));
  LF_HIP(c, hipStreamSynchronize(c->cur));
  *norm = h[0];
  *fault = LF_PLANES_OK, *where = 0;
  if (h[1] != ~0ull)
    *fault = LF_PLANES_ENCODING, *where = (size_t)h[1];
  else if (bound && h[0] > bound)
    *fault = LF_PLANES_BOUND, *where = (size_t)h[2];
  return *fault ? LF_ERR_VERIFICATION : LF_OK;
}

}  // extern "C"
